// vcf_kernels.hip -- the device half of the native VCF reader: the sample columns of a batch of records, as raw text, to packed rows.
//
// k_vcf_gt_pack: one workgroup of 256 lanes per record.  The record's sample columns (`0:186,0:186:99:0,1800<TAB>1:0,147:...`) lie in the
// batch buffer at a 16-byte aligned offset.  The workgroup walks them in steps of 4096 bytes:
//   A. every lane loads 16 consecutive bytes (one dwordx4) and marks its tabs; sixteen 64-bit ballots -- one per byte position -- give each
//      wave the tab pattern of its 1024 bytes: the number of tabs in the lanes below (popcount of the ballots under the lane's own bit) plus
//      the tabs in the lane's own earlier bytes is a tab's rank in the wave, the waves' totals (LDS) and the count carried from the
//      steps before make it the rank in the record = the sample column that STARTS behind that tab.  The starts go to an LDS array.
//   B. the lanes share out the fields that start in this step: skip to FORMAT's GT subfield (colons), reduce it to the three-way code
//      (present as soon as a haplotype is a non-zero allele; otherwise absent if the last haplotype holds a 0, missing if not), look the
//      column up in the column -> sample table and set the bit in the record's present / missing row in LDS (the table permutes: atomic OR).
//      A field may run past the step or the 4096 bytes: the lane reads on in global memory, bounded by the record's length.
// Columns the record does not have (a short line), and every column of a record whose FORMAT has no GT, are missing.  The two rows and
// their popcounts leave with plain vector stores.  k_burden_fold: OR of the present rows of a burden variant's records, the missing row of
// its last record, missing cleared where present (pyseer/input.py:383-407 + 455-503 on one dictionary).
//
// k_bcf_gt_pack: the same rows from BCF records.  A record's GT vector -- n_cols x L values in the int8 coding, (allele + 1) << 1 | phased,
// 0x81 the end of a shorter vector, 0x80 the missing value -- lies in the batch buffer at a 16-byte aligned offset; nothing is tokenised.
// One workgroup per record; a lane takes a column, consecutive lanes consecutive columns (L = 1: one byte, L = 2: one 16-bit load, else a
// loop over L bytes), reduces it by the rule of vcf_gt_code and sets the bit as above.
#include "common.h"
#include "vcf_kernels.h"

#define VCF_WG 256
#define VCF_STEP 4096

__device__ __forceinline__ int vcf_gt_code(const uint8_t *__restrict__ b, uint32_t p, const uint32_t len, const int gi)
{
    int colons = 0;
    while (colons < gi) {
        if (p >= len) return 2;
        const uint8_t c = b[p];
        if (c == '\t') return 2;
        ++p;
        if (c == ':') ++colons;
    }
    bool tok0 = false;                                    // the current (in the end: the last) haplotype holds a 0
    while (p < len) {
        const uint8_t c = b[p];
        if (c == ':' || c == '\t') break;
        if (c == '/' || c == '|') tok0 = false;
        else if (c >= '1' && c <= '9') return 1;
        else if (c == '0') tok0 = true;
        ++p;
    }
    return tok0 ? 0 : 2;
}

__global__ __launch_bounds__(VCF_WG) void k_vcf_gt_pack(const uint8_t *__restrict__ bytes, const ShVcfRec *__restrict__ recs,
                                                        const int32_t *__restrict__ col2idx, const int n_cols, const int row_words,
                                                        uint32_t *__restrict__ present, uint32_t *__restrict__ missing,
                                                        int32_t *__restrict__ n_present, int32_t *__restrict__ n_missing)
{
    extern __shared__ uint32_t s_rows[];                  // [row_words] present, [row_words] missing
    __shared__ uint32_t s_start[VCF_STEP + 1];
    __shared__ uint32_t s_wave[VCF_WG / 64];
    __shared__ int s_cnt[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const ShVcfRec r = recs[blockIdx.x];
    uint32_t *P = s_rows, *M = s_rows + row_words;
    for (int i = tid; i < 2 * row_words; i += VCF_WG) s_rows[i] = 0;
    if (tid < 2) s_cnt[tid] = 0;
    __syncthreads();
    if (r.gt >= 0) {
        const uint8_t *__restrict__ b = bytes + r.off;
        const uint32_t len = r.len;
        const unsigned long long below = (1ull << lane) - 1ull;
        uint32_t fields = 0;                              // fields whose start has been seen in the steps before
        for (uint32_t s0 = 0; s0 == 0 || s0 < len; s0 += VCF_STEP) {
            // ---- A: tabs -> field starts
            const uint32_t my = s0 + (uint32_t)wave * 1024u + (uint32_t)lane * 16u;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (my < len) v = *(const uint4 *)(b + my);   // (16-byte aligned; the batch buffer is padded past its last record)
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            uint32_t mine = 0;                            // bit j: my byte j is a tab inside the record
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (((w[j >> 2] >> (8 * (j & 3))) & 0xffu) == '\t' && my + j < len) mine |= 1u << j;
            uint32_t lower = 0, total = 0;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const unsigned long long m = __ballot((mine >> j) & 1u);
                lower += (uint32_t)__popcll(m & below);
                total += (uint32_t)__popcll(m);
            }
            if (lane == 0) s_wave[wave] = total;
            __syncthreads();
            const uint32_t first = s0 == 0 ? 1u : 0u;     // the record's first field starts at byte 0, behind no tab
            uint32_t base = first, all = first;
#pragma unroll
            for (int k = 0; k < VCF_WG / 64; ++k) { const uint32_t t = s_wave[k]; all += t; if (k < wave) base += t; }
            if (s0 == 0 && tid == 0) s_start[0] = 0;
            uint32_t rank = base + lower;
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if ((mine >> j) & 1u) s_start[rank++] = my + j + 1;
            __syncthreads();
            // ---- B: the fields that start in this step
            for (uint32_t k = tid; k < all; k += VCF_WG) {
                const uint32_t col = fields + k;
                if (col >= (uint32_t)n_cols) break;
                const int idx = col2idx[col];
                if (idx < 0) continue;
                const int code = vcf_gt_code(b, s_start[k], len, r.gt);
                if (code == 1) atomicOr(&P[idx >> 5], 1u << (idx & 31));
                else if (code == 2) atomicOr(&M[idx >> 5], 1u << (idx & 31));
            }
            fields += all;
            __syncthreads();
        }
        for (uint32_t col = fields + tid; col < (uint32_t)n_cols; col += VCF_WG) {       // columns the line does not have
            const int idx = col2idx[col];
            if (idx >= 0) atomicOr(&M[idx >> 5], 1u << (idx & 31));
        }
    } else if (r.gt == -1) {                              // no GT in FORMAT: every sample of the file is missing
        for (int col = tid; col < n_cols; col += VCF_WG) {
            const int idx = col2idx[col];
            if (idx >= 0) atomicOr(&M[idx >> 5], 1u << (idx & 31));
        }
    }                                                     // (gt == -2: a skipped record, rows of zeros)
    __syncthreads();
    int np = 0, nm = 0;
    const size_t row0 = (size_t)blockIdx.x * (size_t)row_words;
    for (int i = tid; i < row_words; i += VCF_WG) {
        const uint32_t p = P[i], m = M[i] & ~p;
        present[row0 + i] = p; missing[row0 + i] = m;
        np += __popc(p); nm += __popc(m);
    }
    if (np) atomicAdd(&s_cnt[0], np);
    if (nm) atomicAdd(&s_cnt[1], nm);
    __syncthreads();
    if (tid == 0) { n_present[blockIdx.x] = s_cnt[0]; n_missing[blockIdx.x] = s_cnt[1]; }
}

// the three-way code of one sample's L values (shvcf::bcf_gt_code, csrc/vcf_reader.cpp, is this function on the host)
__device__ __forceinline__ int bcf_gt_step(const uint32_t b, int &last)
{
    if (b == 0x80u) { last = 2; return 0; }               // the type's missing value
    const int allele = (int)(b >> 1) - 1;
    if (allele >= 1) return 1;
    last = allele == 0 ? 0 : 2;
    return 0;
}

__global__ __launch_bounds__(VCF_WG) void k_bcf_gt_pack(const uint8_t *__restrict__ bytes, const ShVcfRec *__restrict__ recs,
                                                        const int32_t *__restrict__ col2idx, const int n_cols, const int row_words,
                                                        uint32_t *__restrict__ present, uint32_t *__restrict__ missing,
                                                        int32_t *__restrict__ n_present, int32_t *__restrict__ n_missing)
{
    extern __shared__ uint32_t s_rows[];                  // [row_words] present, [row_words] missing
    __shared__ int s_cnt[2];
    const int tid = threadIdx.x;
    const ShVcfRec r = recs[blockIdx.x];
    uint32_t *P = s_rows, *M = s_rows + row_words;
    for (int i = tid; i < 2 * row_words; i += VCF_WG) s_rows[i] = 0;
    if (tid < 2) s_cnt[tid] = 0;
    __syncthreads();
    if (r.gt >= -1) {                                     // (gt == -2: a skipped record, rows of zeros)
        const uint8_t *__restrict__ b = bytes + r.off;
        const uint32_t L = r.len;
        for (int col = tid; col < n_cols; col += VCF_WG) {
            const int idx = col2idx[col];
            if (idx < 0) continue;
            int code = 2, last = 2;                       // no GT in the record: every sample of the file is missing
            if (r.gt >= 0) {
                if (L == 1) {
                    const uint32_t v = b[col];
                    code = v == 0x81u ? 2 : (bcf_gt_step(v, last) ? 1 : last);
                } else if (L == 2) {
                    const uint32_t v = *(const uint16_t *)(b + 2 * (size_t)col), v0 = v & 0xffu, v1 = v >> 8;
                    if (v0 == 0x81u) code = 2;
                    else if (bcf_gt_step(v0, last)) code = 1;
                    else code = v1 == 0x81u ? last : (bcf_gt_step(v1, last) ? 1 : last);
                } else {
                    const uint8_t *__restrict__ q = b + (size_t)col * L;
                    bool hit = false;
                    for (uint32_t j = 0; j < L; ++j) {
                        const uint32_t v = q[j];
                        if (v == 0x81u) break;
                        if (bcf_gt_step(v, last)) { hit = true; break; }
                    }
                    code = hit ? 1 : last;
                }
            }
            if (code == 1) atomicOr(&P[idx >> 5], 1u << (idx & 31));
            else if (code == 2) atomicOr(&M[idx >> 5], 1u << (idx & 31));
        }
    }
    __syncthreads();
    int np = 0, nm = 0;
    const size_t row0 = (size_t)blockIdx.x * (size_t)row_words;
    for (int i = tid; i < row_words; i += VCF_WG) {
        const uint32_t p = P[i], m = M[i] & ~p;
        present[row0 + i] = p; missing[row0 + i] = m;
        np += __popc(p); nm += __popc(m);
    }
    if (np) atomicAdd(&s_cnt[0], np);
    if (nm) atomicAdd(&s_cnt[1], nm);
    __syncthreads();
    if (tid == 0) { n_present[blockIdx.x] = s_cnt[0]; n_missing[blockIdx.x] = s_cnt[1]; }
}

__global__ __launch_bounds__(VCF_WG) void k_burden_fold(const uint32_t *__restrict__ present, const uint32_t *__restrict__ missing, const int row_words,
                                                        const int64_t n_records, const int64_t *__restrict__ csr_off, const int32_t *__restrict__ csr_idx,
                                                        uint32_t *__restrict__ out_present, uint32_t *__restrict__ out_missing,
                                                        int32_t *__restrict__ n_present, int32_t *__restrict__ n_missing)
{
    __shared__ int s_cnt[2];
    const int tid = threadIdx.x;
    if (tid < 2) s_cnt[tid] = 0;
    __syncthreads();
    const int64_t lo = csr_off[blockIdx.x], hi = csr_off[blockIdx.x + 1];
    int np = 0, nm = 0;
    for (int i = tid; i < row_words; i += VCF_WG) {
        uint32_t p = 0, m = 0;
        for (int64_t k = lo; k < hi; ++k) {
            const int64_t rec = csr_idx[k];
            if (rec < 0 || rec >= n_records) continue;
            p |= present[(size_t)rec * row_words + i];
            if (k == hi - 1) m = missing[(size_t)rec * row_words + i];
        }
        m &= ~p;
        out_present[(size_t)blockIdx.x * row_words + i] = p; out_missing[(size_t)blockIdx.x * row_words + i] = m;
        np += __popc(p); nm += __popc(m);
    }
    if (np) atomicAdd(&s_cnt[0], np);
    if (nm) atomicAdd(&s_cnt[1], nm);
    __syncthreads();
    if (tid == 0) { n_present[blockIdx.x] = s_cnt[0]; n_missing[blockIdx.x] = s_cnt[1]; }
}

size_t shk_vcf_lds_bytes(int row_words) { return (size_t)row_words * 8; }

hipError_t shk_vcf_gt_pack(hipStream_t st, const uint8_t *bytes, const ShVcfRec *recs, int64_t n_records, const int32_t *col2idx, int n_cols, int row_words,
                           uint32_t *present, uint32_t *missing, int32_t *n_present, int32_t *n_missing)
{
    if (n_records <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_vcf_gt_pack, dim3((unsigned)n_records), dim3(VCF_WG), shk_vcf_lds_bytes(row_words), st, bytes, recs, col2idx, n_cols, row_words,
                       present, missing, n_present, n_missing);
    return hipGetLastError();
}

hipError_t shk_bcf_gt_pack(hipStream_t st, const uint8_t *bytes, const ShVcfRec *recs, int64_t n_records, const int32_t *col2idx, int n_cols, int row_words,
                           uint32_t *present, uint32_t *missing, int32_t *n_present, int32_t *n_missing)
{
    if (n_records <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_bcf_gt_pack, dim3((unsigned)n_records), dim3(VCF_WG), shk_vcf_lds_bytes(row_words), st, bytes, recs, col2idx, n_cols, row_words,
                       present, missing, n_present, n_missing);
    return hipGetLastError();
}

hipError_t shk_burden_fold(hipStream_t st, const uint32_t *present, const uint32_t *missing, int row_words, int64_t n_records, const int64_t *csr_off,
                           const int32_t *csr_idx, int64_t n_variants, uint32_t *out_present, uint32_t *out_missing, int32_t *n_present, int32_t *n_missing)
{
    if (n_variants <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_burden_fold, dim3((unsigned)n_variants), dim3(VCF_WG), 0, st, present, missing, row_words, n_records, csr_off, csr_idx,
                       out_present, out_missing, n_present, n_missing);
    return hipGetLastError();
}
