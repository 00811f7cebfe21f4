// rtab_kernels.h -- launcher of the Rtab kernel (rtab_kernels.hip) for the entry points in rtab_api.inc.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct ShRtabRec {
    uint64_t off;        // of the line's call text in the batch buffer; a multiple of 16
    uint32_t len;        // bytes of call text
    int32_t has_calls;   // 0: the stripped line holds no tab (status 1)
};

// the kernel's partition of a line, for whoever places test lines on its boundaries (sh_rtab_partition); a step is the lanes' bytes together
#define RTAB_LANE_BYTES 16
#define RTAB_WAVE_BYTES (64 * RTAB_LANE_BYTES)

size_t shk_rtab_lds_bytes(int row_words);
int shk_rtab_default_wg(void);
// wg: lanes per line, 64 (one wavefront) or 256 (one workgroup of four)
hipError_t shk_rtab_pack(hipStream_t st, int wg, const uint8_t *bytes, const ShRtabRec *recs, int64_t n_lines, const int32_t *col2idx, int n_cols, int row_words,
                         uint32_t *present, uint32_t *missing, int32_t *n_present, int32_t *n_missing, int32_t *status);
