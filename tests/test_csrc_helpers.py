"""The device primitives every gfx950 kernel shares have ONE definition, in csrc/pafc_common.h: the 16-byte LDS-DMA, the
round-to-nearest-even bf16 pair conversion, the register-vector typedefs and the exact bf16 pair packing.  Reads the sources,
compiles nothing.  wkv6.hip / wkv6_mfma.inc are exempt: the benchmark keys the scan's measured HBM traffic to the hash of those
two files, so they keep copies of their own (see the header's comment)."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "paper_accurate_fast_cheap_amd", "csrc")
SHARED = "pafc_common.h"
FROZEN = {"wkv6.hip", "wkv6_mfma.inc"}
# vector shapes with one user keep their typedef next to it
OWN_VECTORS = {"gemm_f32.hip": {"f32x16"}, "fbank.hip": {"f32x16"}, "gemm_tn.hip": {"s16x4t", "s16x8t"}}


def _sources():
    paths = [p for ext in ("*.hip", "*.inc", "*.h") for p in glob.glob(os.path.join(CSRC, ext))]
    assert len(paths) > 20 and os.path.join(CSRC, SHARED) in paths
    return {os.path.basename(p): open(p).read() for p in paths if os.path.basename(p) not in FROZEN}


def _files_with(word):
    return sorted(name for name, text in _sources().items() if word in text)


def test_lds_dma_builtin_only_in_the_shared_header():
    assert _files_with("__builtin_amdgcn_global_load_lds") == [SHARED]


def test_convertvector_only_in_the_shared_header():
    assert _files_with("__builtin_convertvector") == [SHARED]


def test_vector_typedefs_only_in_the_shared_header():
    for name, text in _sources().items():
        lines = [ln for ln in text.splitlines() if "ext_vector_type" in ln]
        if name == SHARED:
            assert lines
            continue
        declared = set()
        for ln in lines:
            m = re.match(r"\s*typedef\s+[\w ]+?\s+(\w+)\s+__attribute__\(\(ext_vector_type\(\d+\)\)\);", ln)
            assert m, f"{name}: {ln.strip()}"
            declared.add(m.group(1))
        assert declared == OWN_VECTORS.get(name, set()), name


def test_exact_bf16_pair_packing_only_in_the_shared_header():
    # the body of pack_bf16_exact: (bits(lo) >> 16) | (bits(hi) & 0xffff0000)
    body = re.compile(r"\(__float_as_uint\(\w+\)>>16\)\|\(__float_as_uint\(\w+\)&0xffff0000u?\)")
    hits = sorted(name for name, text in _sources().items() if body.search(re.sub(r"\s+", "", text)))
    assert hits == [SHARED]
