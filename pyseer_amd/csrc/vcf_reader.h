// vcf_reader.h -- the host half of the native VCF reader (vcf_reader.cpp), as the device half (vcf_api.inc, vcf_kernels.hip) sees it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

namespace shvcf {

enum { KEPT = 0, MULTI = 1, FILTERED = 2 };              // skip reasons (include/seerhip.h sh_vcf_next)

struct Record {
    int32_t skip = 0;             // KEPT / MULTI / FILTERED
    int32_t contig = 0;           // id in order of first appearance (Reader::contig_name)
    int64_t pos = 0;              // POS (1-based)
    int32_t ref_len = 0;          // len(REF): the record spans [POS-1, POS-1+ref_len)
    int32_t gt = -1;              // which subfield of FORMAT is GT, -1 = none.  BCF: the values per sample L >= 1 of the GT vector, -1 = none
    const char *name = nullptr; size_t name_len = 0;     // CHROM_POS_REF[_ALT]
    const uint8_t *samp = nullptr; size_t samp_len = 0;  // the sample columns as they stand in the line (after FORMAT's tab, no line end);
                                                         // BCF: the GT vector alone, samp_len = n_cols x L values in the int8 coding
                                                         // both pointers are valid until the next call of next()
};

struct Reader;
Reader *open_file(const char *path, const char *const *sample_names, int n_samples, std::string &err);
void close_file(Reader *r);
int next(Reader *r, Record &rec, std::string &err);      // 1 = a record, 0 = end of file, -1 = error
int n_cols(const Reader *r);                             // sample columns of the #CHROM line
const int32_t *col_to_sample(const Reader *r);           // column -> index in sample_names, -1 = not among them
int n_contigs(const Reader *r);
const char *contig_name(const Reader *r, int id);
int mode(const Reader *r);                               // 0 plain, 1 gzip, 2 BGZF
int format(const Reader *r);                             // 0 VCF text, 1 BCF
// The device kernel's work on the host, one record (k_vcf_gt_pack restated in plain C++: the comparison the rate measurement needs, and the
// check of everything around the kernel where there is no device).  present / missing: row_words zeroed words each.
void host_gt_pack(const uint8_t *samp, size_t len, int gt, const int32_t *col2idx, int n_cols, uint32_t *present, uint32_t *missing, int row_words,
                  int32_t *n_present, int32_t *n_missing);
// The same for a BCF record (k_bcf_gt_pack restated): gt holds n_cols x L values in the int8 coding, sample by sample; has_gt < 0 as
// ShVcfRec::gt (-1: every sample missing, -2: a skipped record).
void host_bcf_pack(const uint8_t *gt, uint32_t L, int has_gt, const int32_t *col2idx, int n_cols, uint32_t *present, uint32_t *missing, int row_words,
                   int32_t *n_present, int32_t *n_missing);

}  // namespace shvcf
