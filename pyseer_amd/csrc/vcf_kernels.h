// vcf_kernels.h -- launchers of the VCF kernels (vcf_kernels.hip) for the entry points in vcf_api.inc.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct ShVcfRec {
    uint64_t off;        // of the record's sample columns in the batch buffer; a multiple of 16
    uint32_t len;        // bytes of sample columns.  BCF: the values per sample L of the GT vector (n_cols x L bytes at off)
    int32_t gt;          // which subfield of FORMAT is GT; -1 none (all missing); -2 a skipped record (rows of zeros).  BCF: >= 0 a GT vector
};

size_t shk_vcf_lds_bytes(int row_words);
hipError_t shk_vcf_gt_pack(hipStream_t st, const uint8_t *bytes, const ShVcfRec *recs, int64_t n_records, const int32_t *col2idx, int n_cols, int row_words,
                           uint32_t *present, uint32_t *missing, int32_t *n_present, int32_t *n_missing);
hipError_t shk_bcf_gt_pack(hipStream_t st, const uint8_t *bytes, const ShVcfRec *recs, int64_t n_records, const int32_t *col2idx, int n_cols, int row_words,
                           uint32_t *present, uint32_t *missing, int32_t *n_present, int32_t *n_missing);
hipError_t shk_burden_fold(hipStream_t st, const uint32_t *present, const uint32_t *missing, int row_words, int64_t n_records, const int64_t *csr_off,
                           const int32_t *csr_idx, int64_t n_variants, uint32_t *out_present, uint32_t *out_missing, int32_t *n_present, int32_t *n_missing);
