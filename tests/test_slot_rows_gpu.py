"""pafc_rows_gather / pafc_rows_scatter (hip_ops.RowsTable): rows of many tensors between the slots of a pool and a dense
batch, one launch each way, against torch indexing; padding rows, unnamed slots and guard rows behind every tensor."""
import pytest
import torch

pytestmark = pytest.mark.gpu
S = 5
# bytes per row: 12 (the 4-byte path), 1 024 ("shift"), 14 336 ("cnn", C = 512, lorder 14), 131 072 ("wkv")
SHAPES = [((3,), torch.float32), ((1, 512), torch.bfloat16), ((512, 14), torch.bfloat16), ((8, 64, 64), torch.float32)]
CASES = [[3], [4, 0, 2], [2, -1, 4, 1]]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _tensors(rows, seed, shift=0):
    """Every tensor with a guard row behind it (and `shift` elements in front: a base that is not 16-byte aligned)."""
    g = torch.Generator().manual_seed(seed)
    full, views = [], []
    for shape, dt in SHAPES:
        n = 1
        for d in shape:
            n *= d
        flat = torch.randn(shift + (rows + 1) * n, generator=g).to(dt).cuda()
        full.append(flat)
        views.append(flat[shift:shift + rows * n].view((rows,) + shape))
    return full, views


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("idx", CASES, ids=["m1", "m3", "m4_one_padding_row"])
def test_gather_and_scatter_equal_torch_indexing(hip, idx, shift):
    from paper_accurate_fast_cheap_amd.hip_ops import RowsTable
    m = len(idx)
    pool_full, pool = _tensors(S, 1, shift if shift == 0 else 2)       # (2 bf16 = 1 fp32 element = 4 bytes off)
    comp_full, comp = _tensors(m, 2, shift if shift == 0 else 2)
    if shift:
        assert all(p.data_ptr() % 16 != 0 and p.data_ptr() % 4 == 0 for p in pool)
    table = RowsTable(list(zip(pool, comp)))
    dev_idx = torch.tensor(idx, dtype=torch.int32).cuda()
    live = [j for j, s in enumerate(idx) if s >= 0]
    sel = torch.tensor([idx[j] for j in live]).cuda()
    pool0 = [f.clone() for f in pool_full]
    comp0 = [f.clone() for f in comp_full]
    table.gather(dev_idx, m)
    for p, c, pf, p0, cf, c0 in zip(pool, comp, pool_full, pool0, comp_full, comp0):
        assert torch.equal(_bits(c[live]), _bits(p.index_select(0, sel)))
        for j, s in enumerate(idx):
            if s < 0:
                assert int(_bits(c[j]).ne(0).sum()) == 0              # a padding row is zeros
        assert torch.equal(_bits(pf), _bits(p0))                      # the pool is read only
        n = c[0].numel()
        front = cf.numel() - (m + 1) * n
        assert torch.equal(_bits(cf[-n:]), _bits(c0[-n:])) and torch.equal(_bits(cf[:front]), _bits(c0[:front]))   # its guards
    # new compact rows, scattered back
    _, fresh = _tensors(m, 3)
    for c, f in zip(comp, fresh):
        c.copy_(f)
    table.scatter(dev_idx, m)
    for p, c, pf, p0 in zip(pool, comp, pool_full, pool0):
        assert torch.equal(_bits(p.index_select(0, sel)), _bits(c[live]))
        rest = [s for s in range(S) if s not in idx]
        n = p[0].numel()
        front = pf.numel() - (S + 1) * n
        was = p0[front:front + S * n].view_as(p)
        assert torch.equal(_bits(p[rest]), _bits(was[rest]))          # every other slot
        assert torch.equal(_bits(pf[-n:]), _bits(p0[-n:])) and torch.equal(_bits(pf[:front]), _bits(p0[:front]))   # the guards


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_feature_windows_out_of_the_ring_ride_in_the_same_launch(hip, dtype):
    from paper_accurate_fast_cheap_amd.hip_ops import RowsTable
    ring_frames, window, F = 96, 67, 80
    g = torch.Generator().manual_seed(5)
    ring = torch.randn(S, ring_frames, F, generator=g).to(dtype).cuda()
    state = torch.randn(S, 1, 128, generator=g).cuda()
    idx, starts = [4, -1, 0, 2], [50, 0, 1000, 29]                   # 50 + 67 wraps; 1000 mod 96 = 40 wraps too; 29 + 67 == 96
    xs = torch.full((len(idx) + 1, window, F), 7.0, dtype=dtype).cuda()
    comp = torch.empty(len(idx), 1, 128).cuda()
    table = RowsTable([(state, comp)], [(ring, xs[:len(idx)])])
    assert table.frame_bytes == F * ring.element_size()
    offs = torch.tensor([(s % ring_frames) * table.frame_bytes for s in starts], dtype=torch.int32).cuda()
    table.gather(torch.tensor(idx, dtype=torch.int32).cuda(), len(idx), offs)
    for j, (s, a) in enumerate(zip(idx, starts)):
        if s < 0:
            assert int(_bits(xs[j]).ne(0).sum()) == 0 and int(_bits(comp[j]).ne(0).sum()) == 0
            continue
        rows = [(a + k) % ring_frames for k in range(window)]
        assert torch.equal(_bits(xs[j]), _bits(ring[s, rows])), j
        assert torch.equal(comp[j], state[s])
    assert bool((xs[-1] == 7.0).all())                                # the guard row


def test_rows_table_refuses_bad_operands(hip):
    from paper_accurate_fast_cheap_amd._lib import PafcError
    from paper_accurate_fast_cheap_amd.hip_ops import RowsTable
    pool, comp = torch.zeros(S, 8).cuda(), torch.zeros(3, 8).cuda()
    with pytest.raises(PafcError, match="row shapes differ"):
        RowsTable([(pool, torch.zeros(3, 9).cuda())])
    with pytest.raises(PafcError, match="no CPU fallback"):
        RowsTable([(pool.cpu(), comp.cpu())])
    with pytest.raises(PafcError, match="bad dims"):                 # 6-byte rows
        RowsTable([(torch.zeros(S, 3, dtype=torch.bfloat16).cuda(), torch.zeros(3, 3, dtype=torch.bfloat16).cuda())]).gather(
            torch.zeros(3, dtype=torch.int32).cuda(), 3)
    t = RowsTable([(pool, comp)])
    with pytest.raises(PafcError, match="the compact tensors hold 3"):
        t.gather(torch.zeros(4, dtype=torch.int32).cuda(), 4)
    with pytest.raises(PafcError, match="int32"):
        t.scatter(torch.zeros(3, dtype=torch.int64).cuda(), 3)
