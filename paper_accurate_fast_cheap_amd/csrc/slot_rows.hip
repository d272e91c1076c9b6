// Rows of many tensors between a pool of S slots and a dense batch of m rows, ONE launch per direction (C ABI:
// pafc_rows_gather / pafc_rows_scatter in include/pafc_encoder_ops.h).
//
// A streaming encoder step takes a dense batch, a server's streams sit in slots: before a step the carries of the m
// streams that run are brought together, after it they are put back.  With framework ops that is one index_select and one
// index_copy_ per carry tensor (36 tensors in a 12-layer model).  Here a table of {pool base, compact base, row bytes,
// ring bytes} entries is walked by one grid (16 KiB pieces of a row, m rows, entries); idx (m) in device memory names the slot
// of every compact row, so a captured launch serves any choice of slots.  Plain coalesced copies: 16 bytes per lane where
// bases and sizes allow, 4 bytes otherwise.  A ring entry (ring bytes > 0) reads row j's bytes from offs[j] on in its slot's
// ring of that many bytes, wrapping: the feature window of a stream out of the ring pafc_fbank_stream_rows writes.
#include "pafc_common.h"
#include "../../include/pafc_encoder_ops.h"

namespace pafc {
namespace {

constexpr long PIECE = 16384;       // bytes of a row one block moves
constexpr int ENTRY = 4;            // longs per table entry

template <bool SCATTER>
__global__ __launch_bounds__(256) void slot_rows_kernel(const long *table, const int *idx, const int *offs, int S) {
    const long *e = table + ENTRY * blockIdx.z;
    const long rb = e[2], ring = e[3];
    const long x0 = (long)blockIdx.x * PIECE;
    if (x0 >= rb) return;
    const long x1 = x0 + PIECE < rb ? x0 + PIECE : rb;
    const int j = blockIdx.y, s = idx[j];
    if (s >= S) return;                                // never outside the pool, whatever idx holds
    char *comp = (char *)e[1] + (long)j * rb;
    const int tid = threadIdx.x;
    if (s < 0) {                                       // a padding row: zeros in, nothing out
        if (SCATTER) return;
        if ((((long)comp | rb) & 15) == 0) {
            for (long x = x0 + 16 * tid; x < x1; x += 16 * 256) *(uint4 *)(comp + x) = make_uint4(0, 0, 0, 0);
        } else {
            for (long x = x0 + 4 * tid; x < x1; x += 4 * 256) *(uint32_t *)(comp + x) = 0u;
        }
        return;
    }
    if (ring == 0) {
        char *pool = (char *)e[0] + (long)s * rb;
        char *dst = SCATTER ? pool : comp;
        const char *src = SCATTER ? comp : pool;
        if ((((long)pool | (long)comp | rb) & 15) == 0) {
            for (long x = x0 + 16 * tid; x < x1; x += 16 * 256) *(uint4 *)(dst + x) = *(const uint4 *)(src + x);
        } else {
            for (long x = x0 + 4 * tid; x < x1; x += 4 * 256) *(uint32_t *)(dst + x) = *(const uint32_t *)(src + x);
        }
        return;
    }
    if (SCATTER) return;                               // (refused on the host: a ring is filled by the fbank)
    const char *pool = (const char *)e[0] + (long)s * ring;
    long off = offs[j];
    off = off < 0 ? 0 : off % ring;
    if ((((long)pool | (long)comp | rb | ring | off) & 15) == 0) {
        for (long x = x0 + 16 * tid; x < x1; x += 16 * 256) *(uint4 *)(comp + x) = *(const uint4 *)(pool + (off + x) % ring);
    } else {
        for (long x = x0 + 4 * tid; x < x1; x += 4 * 256) *(uint32_t *)(comp + x) = *(const uint32_t *)(pool + (off + x) % ring);
    }
}

// table: the host copy.  -> PAFC_OK and the largest row, or the error
int check(const long *table, const void *table_dev, int n, const void *idx, const void *offs, int m, int S, bool scatter,
          long *max_row) {
    if (!table || !table_dev || !idx) return PAFC_ERR_NULL_POINTER;
    if (n <= 0 || n > 65535 || m <= 0 || m > 65535 || S <= 0) return PAFC_ERR_BAD_DIMS;
    long most = 0;
    for (int i = 0; i < n; ++i) {
        const long pool = table[ENTRY * i], comp = table[ENTRY * i + 1], rb = table[ENTRY * i + 2], ring = table[ENTRY * i + 3];
        if (!pool || !comp) return PAFC_ERR_NULL_POINTER;
        if (rb <= 0 || (rb & 3) || ring < 0 || (ring & 3) || (ring && ring < rb)) return PAFC_ERR_BAD_DIMS;
        if ((pool | comp) & 3) return PAFC_ERR_ALIGNMENT;
        if (ring && scatter) return PAFC_ERR_UNSUPPORTED;
        if (ring && !offs) return PAFC_ERR_NULL_POINTER;
        most = rb > most ? rb : most;
    }
    if ((most + PIECE - 1) / PIECE > 0x7fffffffL) return PAFC_ERR_BAD_DIMS;
    *max_row = most;
    return PAFC_OK;
}

template <bool SCATTER>
int launch(const long *table, const long *table_dev, int n, const int *idx, const int *offs, int m, int S, hipStream_t stream) {
    long most = 0;
    const int rc = check(table, table_dev, n, idx, offs, m, S, SCATTER, &most);
    if (rc != PAFC_OK) return rc;
    const dim3 grid((unsigned)((most + PIECE - 1) / PIECE), (unsigned)m, (unsigned)n);
    hipLaunchKernelGGL((slot_rows_kernel<SCATTER>), grid, dim3(256), 0, stream, table_dev, idx, offs, S);
    return hipGetLastError() == hipSuccess ? PAFC_OK : PAFC_ERR_LAUNCH;
}

}  // namespace
}  // namespace pafc

extern "C" {

int pafc_rows_gather(const long *table, const long *table_dev, int n, const int *idx, const int *offs, int m, int S,
                     pafc_stream_t stream) {
    return pafc::launch<false>(table, table_dev, n, idx, offs, m, S, (hipStream_t)stream);
}

int pafc_rows_scatter(const long *table, const long *table_dev, int n, const int *idx, int m, int S, pafc_stream_t stream) {
    return pafc::launch<true>(table, table_dev, n, idx, nullptr, m, S, (hipStream_t)stream);
}

}  // extern "C"
