// rtab_kernels.hip -- the device half of the native Rtab reader: the call text of a batch of lines (`1<TAB>0<TAB><TAB>.<TAB>1 ...`) to packed rows.
//
// k_rtab_pack<WG>: WG lanes per line (64: one wavefront, 256: a workgroup of four).  The line's call text lies in the batch buffer at a 16-byte
// aligned offset, padded to 16 bytes.  A call is at most one byte, so there is nothing to walk: every byte is judged where it was loaded.
// The lanes take the text in steps of WG * 16 bytes:
//   * every lane loads 16 consecutive bytes (one dwordx4) plus the byte in front of them and the byte behind them (a lane's first and last
//     byte have their neighbours in another lane, wavefront or step), and marks its tabs;
//   * a byte's column is the number of tabs in front of it in the line: sixteen 64-bit ballots -- one per byte position -- give each wavefront
//     the tab pattern of its 1024 bytes; the popcount of the ballots under the lane's own bit counts the tabs of the lanes below, the
//     wavefronts' totals go through LDS (two slots by step parity: one barrier per step), the count of the steps before is carried;
//   * a byte that is no tab is a call only if both neighbours are a tab or an end of the line; then `1` sets the column's bit in the present
//     row, `.` in the missing row, `0` nothing, and anything else -- like a token of two bytes or more -- makes the line "not binary";
//   * a tab behind a tab or at the start of the line closes an empty call (missing) in its column, a tab at the end of the line opens one
//     in the next;
//   * the bits go into the two rows in LDS with atomic OR (the column -> sample table permutes); rows, counts and status leave with plain
//     vector stores.
// Status (the reference's order of checks, pyseer/input.py:377-383): 1 no calls, 2 the number of calls (tabs + 1) is not the header's,
// 3 not binary -- in any column, with or without a phenotype.  The rows of a line whose status is not 0 leave as zeros.
//
// One wavefront or one workgroup per line: both are built (the route key rtab_wg picks one, for the tests and the measurement); the
// default is a workgroup of 256, by measurement (tools/bench_rtab_reader.py, profiles/r12/rtab_reader.txt; N = 5000, lines of 10.3 KB,
// ~2860 lines per launch): the kernel alone takes 105 us per launch with a workgroup per line against 124 us with a wavefront per line
// (27.3 against 23.0 M lines/s) -- a line is 3 steps of a workgroup but 11 of a wavefront, each with its ballots and its barrier.  End to
// end the two are not told apart (812 k against 780 k lines/s, inside the spread of the passes): the host's framing and copies bind.
#include "common.h"
#include "rtab_kernels.h"

#define RTAB_WG_DEFAULT 256

template <int WG>
__global__ __launch_bounds__(WG) void k_rtab_pack(const uint8_t *__restrict__ bytes, const ShRtabRec *__restrict__ recs, const int32_t *__restrict__ col2idx,
                                                  const int n_cols, const int row_words, uint32_t *__restrict__ present, uint32_t *__restrict__ missing,
                                                  int32_t *__restrict__ n_present, int32_t *__restrict__ n_missing, int32_t *__restrict__ status)
{
    constexpr int WAVES = WG / 64;
    constexpr uint32_t STEP = (uint32_t)WG * RTAB_LANE_BYTES;
    extern __shared__ uint32_t s_rows[];                  // [row_words] present, [row_words] missing
    __shared__ uint32_t s_wave[2][WAVES];
    __shared__ int s_cnt[2];
    __shared__ int s_bad;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const ShRtabRec r = recs[blockIdx.x];
    uint32_t *P = s_rows, *M = s_rows + row_words;
    for (int i = tid; i < 2 * row_words; i += WG) s_rows[i] = 0;
    if (tid < 2) s_cnt[tid] = 0;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    int st = 0;
    if (!r.has_calls) st = 1;
    else {
        const uint8_t *__restrict__ b = bytes + r.off;
        const uint32_t len = r.len;
        const unsigned long long below = (1ull << lane) - 1ull;
        uint32_t tabs = 0;                                // tabs in the steps before
        bool bad = false;
        int par = 0;
        for (uint32_t s0 = 0; s0 < len; s0 += STEP, par ^= 1) {
            const uint32_t my = s0 + (uint32_t)wave * RTAB_WAVE_BYTES + (uint32_t)lane * RTAB_LANE_BYTES;
            uint4 v = make_uint4(0, 0, 0, 0);
            uint32_t before = '\t', behind = '\t';        // an end of the line stands for a tab
            if (my < len) {
                v = *(const uint4 *)(b + my);             // (16-byte aligned; the line is padded to 16 bytes)
                if (my > 0) before = b[my - 1];
                if (my + RTAB_LANE_BYTES < len) behind = b[my + RTAB_LANE_BYTES];
            }
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            const uint32_t mine_n = my < len ? min(len - my, (uint32_t)RTAB_LANE_BYTES) : 0u;      // my bytes inside the line
            uint32_t mine = 0;                            // bit j: my byte j is a tab inside the line
#pragma unroll
            for (int j = 0; j < RTAB_LANE_BYTES; ++j)
                if (((w[j >> 2] >> (8 * (j & 3))) & 0xffu) == '\t' && (uint32_t)j < mine_n) mine |= 1u << j;
            uint32_t lower = 0, total = 0;
#pragma unroll
            for (int j = 0; j < RTAB_LANE_BYTES; ++j) {
                const unsigned long long m = __ballot((mine >> j) & 1u);
                lower += (uint32_t)__popcll(m & below);
                total += (uint32_t)__popcll(m);
            }
            if (lane == 0) s_wave[par][wave] = total;
            __syncthreads();
            uint32_t col = tabs + lower;
#pragma unroll
            for (int k = 0; k < WAVES; ++k) { const uint32_t t = s_wave[par][k]; tabs += t; if (k < wave) col += t; }
            uint32_t prev = before;
#pragma unroll
            for (int j = 0; j < RTAB_LANE_BYTES; ++j) {
                const uint32_t c = (w[j >> 2] >> (8 * (j & 3))) & 0xffu;
                if ((uint32_t)j < mine_n) {
                    const bool last = (uint32_t)j + 1 == mine_n;                                   // my last byte inside the line
                    const uint32_t in_lane = j + 1 < RTAB_LANE_BYTES ? (w[((j + 1) & 15) >> 2] >> (8 * ((j + 1) & 3))) & 0xffu : behind;
                    const uint32_t next = last ? behind : in_lane;
                    int code = 0;                         // 1 present, 2 missing: for column `col`
                    if (c == '\t') {
                        if (prev == '\t') code = 2;       // an empty call ends here
                    } else if (prev != '\t' || next != '\t') bad = true;
                    else if (c == '1') code = 1;
                    else if (c == '.') code = 2;
                    else if (c != '0') bad = true;
                    if (code && col < (uint32_t)n_cols) {
                        const int idx = col2idx[col];
                        if (idx >= 0) atomicOr(code == 1 ? &P[idx >> 5] : &M[idx >> 5], 1u << (idx & 31));
                    }
                    if (c == '\t') {
                        ++col;
                        if (my + (uint32_t)j + 1 == len && col < (uint32_t)n_cols) {              // a tab ends the line: one more empty call
                            const int idx = col2idx[col];
                            if (idx >= 0) atomicOr(&M[idx >> 5], 1u << (idx & 31));
                        }
                    }
                }
                prev = c;
            }
        }
        if (len == 0 && tid == 0 && n_cols == 1 && col2idx[0] >= 0) M[col2idx[0] >> 5] = 1u << (col2idx[0] & 31);      // one empty call
        if (bad) s_bad = 1;
        __syncthreads();
        st = tabs + 1u != (uint32_t)n_cols ? 2 : (s_bad ? 3 : 0);
    }
    __syncthreads();
    int np = 0, nm = 0;
    const size_t row0 = (size_t)blockIdx.x * (size_t)row_words;
    for (int i = tid; i < row_words; i += WG) {
        const uint32_t p = st ? 0u : P[i], m = st ? 0u : M[i] & ~p;
        present[row0 + i] = p; missing[row0 + i] = m;
        np += __popc(p); nm += __popc(m);
    }
    if (np) atomicAdd(&s_cnt[0], np);
    if (nm) atomicAdd(&s_cnt[1], nm);
    __syncthreads();
    if (tid == 0) { n_present[blockIdx.x] = s_cnt[0]; n_missing[blockIdx.x] = s_cnt[1]; status[blockIdx.x] = st; }
}

size_t shk_rtab_lds_bytes(int row_words) { return (size_t)row_words * 8; }
int shk_rtab_default_wg(void) { return RTAB_WG_DEFAULT; }

hipError_t shk_rtab_pack(hipStream_t st, int wg, const uint8_t *bytes, const ShRtabRec *recs, int64_t n_lines, const int32_t *col2idx, int n_cols, int row_words,
                         uint32_t *present, uint32_t *missing, int32_t *n_present, int32_t *n_missing, int32_t *status)
{
    if (n_lines <= 0) return hipSuccess;
    if (wg == 0) wg = RTAB_WG_DEFAULT;
    if (wg == 64)
        hipLaunchKernelGGL(k_rtab_pack<64>, dim3((unsigned)n_lines), dim3(64), shk_rtab_lds_bytes(row_words), st, bytes, recs, col2idx, n_cols, row_words,
                           present, missing, n_present, n_missing, status);
    else if (wg == 256)
        hipLaunchKernelGGL(k_rtab_pack<256>, dim3((unsigned)n_lines), dim3(256), shk_rtab_lds_bytes(row_words), st, bytes, recs, col2idx, n_cols, row_words,
                           present, missing, n_present, n_missing, status);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}
