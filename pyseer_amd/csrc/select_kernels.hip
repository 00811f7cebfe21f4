// select_kernels.hip -- a packed cache served to a subset or another order of its samples: the rows of a block over n_src samples become rows
// over n_dst of them, bit j of a new row = bit map[j] of the old one.
//
// k_rows_select<R>: one wavefront per R consecutive rows, blockDim.x / 64 wavefronts per workgroup.
//   * the wavefront's R source rows are contiguous in memory: they go to the wavefront's own part of the LDS as they stand, 8 bytes per lane
//     and step (rows are 8-byte aligned: row_bytes_for), pad bits included -- nothing below reads them, since every map entry is < n_src;
//   * step w makes output word w (64 bits) of all R rows: lane l loads map[64 w + l] once (coalesced; the table is shared by every row and
//     stays in the caches) and picks that bit of each of the R rows from the LDS; a ballot per row is the output word, which lane w & 63
//     keeps in a register; lanes with 64 w + l >= n_dst vote 0, so the pad bits of the ragged last word are zeros;
//   * after 64 steps, and after the last, the kept words leave with one coalesced 8-byte store per lane and row;
//   * a row's count is the sum of the popcounts of its ballots.
// R = 4 shares a map load between four rows (the table is 4 n_dst bytes against n_src / 8 of a row: with one row per wavefront the table
// is 30 times the row's own traffic); a source row too wide for sixteen rows per workgroup in 64 KB of LDS takes R = 1 with four
// wavefronts, then one wavefront; wider than 64 KB is refused by the caller (shk_rows_select_max_row_bytes).
// All stores are plain vector stores; the map is validated by the host (csrc/select_api.inc) before it is uploaded.
#include "common.h"

#define SELECT_LDS_MAX 65536

template <int R>
__global__ __launch_bounds__(256) void k_rows_select(const uint64_t *__restrict__ src, const int src_words, const int64_t V, const int32_t *__restrict__ map,
                                                     const int n_dst, const int out_words, uint64_t *__restrict__ out, int32_t *__restrict__ counts)
{
    extern __shared__ uint64_t s_sel[];                   // [wavefronts][R][src_words]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const int64_t row0 = ((int64_t)blockIdx.x * waves + wave) * R;
    const int nr = row0 < V ? (int)min((int64_t)R, V - row0) : 0;      // rows of this wavefront (0: a wavefront behind the last row)
    uint64_t *mine = s_sel + (size_t)wave * R * src_words;
    const uint64_t *from = src + (size_t)row0 * src_words;
    for (int i = lane; i < nr * src_words; i += 64) mine[i] = from[i];
    __syncthreads();
    if (nr == 0) return;
    const uint32_t *m32 = (const uint32_t *)mine;         // (little-endian: bit m of a row is bit m & 31 of its 32-bit word m >> 5)
    uint64_t keep[R];
    int cnt[R];
#pragma unroll
    for (int r = 0; r < R; ++r) { keep[r] = 0; cnt[r] = 0; }
    for (int w = 0; w < out_words; ++w) {
        const int j = 64 * w + lane;
        const bool in = j < n_dst;
        const int m = in ? map[j] : 0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            // (a row at or behind nr was not staged: what it reads lies inside the wavefront's own LDS and is never stored)
            const uint32_t word = m32[(size_t)r * src_words * 2 + (m >> 5)];
            const unsigned long long b = __ballot(in && ((word >> (m & 31)) & 1u));
            cnt[r] += __popcll(b);
            if (lane == (w & 63)) keep[r] = b;
        }
        if ((w & 63) == 63 || w == out_words - 1) {
            const int base = w & ~63;
            if (base + lane <= w) {
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (r < nr) out[(size_t)(row0 + r) * out_words + base + lane] = keep[r];
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (r < nr) counts[row0 + r] = cnt[r];
    }
}

extern "C" {

int64_t shk_rows_select_max_row_bytes(void) { return SELECT_LDS_MAX; }

// src: V rows of src_row_bytes (a multiple of 8, at most shk_rows_select_max_row_bytes()), 8-byte aligned; map: n_dst entries, each below
// src_row_bytes * 8; out: V rows of ((n_dst + 63) / 64) * 8 bytes; counts: V entries
hipError_t shk_rows_select(hipStream_t st, const void *src, int64_t src_row_bytes, int64_t V, const int32_t *map, int n_dst, void *out, int32_t *counts)
{
    if (V <= 0) return hipSuccess;
    if (src_row_bytes <= 0 || (src_row_bytes & 7) || src_row_bytes > SELECT_LDS_MAX || n_dst < 1 || (((uintptr_t)src | (uintptr_t)out) & 7)) return hipErrorInvalidValue;
    const int src_words = (int)(src_row_bytes >> 3), out_words = (n_dst + 63) >> 6;
    if (16 * src_row_bytes <= SELECT_LDS_MAX) {
        const int64_t blocks = (V + 15) / 16;
        hipLaunchKernelGGL(k_rows_select<4>, dim3((unsigned)blocks), dim3(256), (size_t)(16 * src_row_bytes), st, (const uint64_t *)src, src_words, V, map, n_dst,
                           out_words, (uint64_t *)out, counts);
    } else {
        const int waves = 4 * src_row_bytes <= SELECT_LDS_MAX ? 4 : 1;
        const int64_t blocks = (V + waves - 1) / waves;
        hipLaunchKernelGGL(k_rows_select<1>, dim3((unsigned)blocks), dim3(64 * waves), (size_t)(waves * src_row_bytes), st, (const uint64_t *)src, src_words, V, map,
                           n_dst, out_words, (uint64_t *)out, counts);
    }
    return hipGetLastError();
}

}  // extern "C"
