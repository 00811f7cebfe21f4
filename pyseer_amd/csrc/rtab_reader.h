// rtab_reader.h -- the host half of the native Rtab reader (rtab_reader.cpp), as the device half (rtab_api.inc, rtab_kernels.hip) sees it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

namespace shrtab {

enum { OK = 0, NO_CALLS = 1, MISMATCH = 2, NOT_BINARY = 3 };   // row status (include/seerhip.h sh_rtab_next)

struct Line {
    const char *name = nullptr; size_t name_len = 0;     // everything before the first tab (the whole stripped line if it has none)
    const uint8_t *calls = nullptr; size_t calls_len = 0;  // the text behind the first tab as it stands, trailing strip applied
    bool has_calls = false;                                // the stripped line holds a tab
};                                                         // (the pointers stay valid until close_file: they point into the file's mapping)

struct Reader;
// columns: the header's sample columns as the caller split them (the first line of the file is skipped, not parsed).  dup: set when a
// phenotype sample is named by more than one column -- the reader refuses such a table (err says which sample).
Reader *open_file(const char *path, const char *const *sample_names, int n_samples, const char *const *columns, int n_columns, std::string &err, bool &dup);
void close_file(Reader *r);
int next(Reader *r, Line &line);                         // 1 = a line, 0 = end of file
int n_cols(const Reader *r);
const int32_t *col_to_sample(const Reader *r);           // column -> index in sample_names, -1 = not among them
// The device kernel's work on the host, one line (k_rtab_pack restated in plain C++ by splitting at tabs: what runs where there is no
// device, and the other side of the rate comparison).  present / missing: row_words zeroed words each; returns the status, and leaves the
// rows zero unless it is OK.
int host_rtab_pack(const uint8_t *calls, size_t len, bool has_calls, const int32_t *col2idx, int n_cols, uint32_t *present, uint32_t *missing, int row_words,
                   int32_t *n_present, int32_t *n_missing);

}  // namespace shrtab
