// rtab_reader.cpp -- native Rtab reader, host half: the reference reads a presence/absence table line by line (pyseer/input.py:301-454,
// the 'Rtab' branch of read_variant): `line.rstrip().split('\t')`, the first field the name, the others one call per header column.  This
// reader frames the file exactly as Python's text mode does and hands out, per line, the name and the call text as it stands; the calls --
// all but a few bytes of a line -- are NOT tokenised here: csrc/rtab_api.inc sends them to the device (k_rtab_pack, csrc/rtab_kernels.hip).
//   * plain text only (what open(var_file) reads); the first line is the header, which the caller has split already;
//   * a line ends at \n, \r\n or a lone \r; a last line without a terminator is a line; an empty line is a line without fields;
//   * the end of a line is stripped of what str.rstrip() strips among ASCII bytes: 0x09-0x0d, 0x1c-0x1f, 0x20 -- trailing empty calls go
//     with it, as they do in the reference;
//   * the name is everything before the first tab: it may hold spaces and may be empty.
// Not covered: non-ASCII whitespace at the end of a line (U+0085, U+00A0, ... -- str.rstrip() strips those too) and bytes that are not UTF-8
// (the reference raises UnicodeDecodeError).
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstring>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "rtab_reader.h"

namespace shrtab {

struct Reader {
    int fd = -1; const uint8_t *map = nullptr; size_t map_len = 0;
    size_t pos = 0;                                       // the next unread byte
    size_t nl = 0; bool nl_known = false;                 // the first \n at or behind pos (map_len: none), once it has been looked for
    std::vector<int32_t> col2idx;
    ~Reader() { if (map && map_len) munmap((void *)map, map_len); if (fd >= 0) ::close(fd); }
};

// the next line as Python's universal newlines frame it, without its terminator; false at the end of the file
static bool next_line(Reader *r, const uint8_t *&line, size_t &len)
{
    if (r->pos >= r->map_len) return false;
    const uint8_t *const base = r->map;
    if (!r->nl_known || r->nl < r->pos) {
        const void *q = memchr(base + r->pos, '\n', r->map_len - r->pos);
        r->nl = q ? (size_t)((const uint8_t *)q - base) : r->map_len;
        r->nl_known = true;
    }
    line = base + r->pos;
    const void *q = memchr(line, '\r', r->nl - r->pos);
    if (q) {                                              // \r\n, or a lone \r in front of the next \n
        const size_t cr = (size_t)((const uint8_t *)q - base);
        len = cr - r->pos;
        r->pos = (cr + 1 == r->nl && r->nl < r->map_len) ? r->nl + 1 : cr + 1;
    } else {
        len = r->nl - r->pos;
        r->pos = r->nl < r->map_len ? r->nl + 1 : r->map_len;
    }
    return true;
}

static inline bool ascii_space(uint8_t c) { return (c >= 0x09 && c <= 0x0d) || (c >= 0x1c && c <= 0x20); }

Reader *open_file(const char *path, const char *const *sample_names, int n_samples, const char *const *columns, int n_columns, std::string &err, bool &dup)
{
    dup = false;
    std::unique_ptr<Reader> r(new Reader());
    r->fd = ::open(path, O_RDONLY);
    struct stat st;
    if (r->fd < 0 || fstat(r->fd, &st) != 0) { err = std::string("cannot open ") + path; return nullptr; }
    r->map_len = (size_t)st.st_size;
    if (r->map_len) {
        void *m = mmap(nullptr, r->map_len, PROT_READ, MAP_PRIVATE, r->fd, 0);
        if (m == MAP_FAILED) { r->map_len = 0; err = std::string("cannot map ") + path; return nullptr; }
        r->map = (const uint8_t *)m;
        madvise(m, r->map_len, MADV_SEQUENTIAL);
    }
    std::unordered_map<std::string, int> sample_idx;
    for (int i = 0; i < n_samples; ++i) sample_idx.emplace(sample_names[i], i);
    std::vector<char> seen((size_t)n_samples, 0);
    r->col2idx.reserve((size_t)n_columns);
    for (int c = 0; c < n_columns; ++c) {
        auto it = sample_idx.find(columns[c]);
        const int idx = it == sample_idx.end() ? -1 : it->second;
        if (idx >= 0) {
            if (seen[(size_t)idx]) { dup = true; err = std::string("Rtab: duplicate sample column ") + columns[c]; return nullptr; }
            seen[(size_t)idx] = 1;
        }
        r->col2idx.push_back(idx);
    }
    const uint8_t *line; size_t len;
    next_line(r.get(), line, len);                        // the header
    return r.release();
}

void close_file(Reader *r) { delete r; }
int n_cols(const Reader *r) { return (int)r->col2idx.size(); }
const int32_t *col_to_sample(const Reader *r) { return r->col2idx.data(); }

int next(Reader *r, Line &out)
{
    const uint8_t *line; size_t len;
    if (!next_line(r, line, len)) return 0;
    while (len && ascii_space(line[len - 1])) --len;
    const uint8_t *t = len ? (const uint8_t *)memchr(line, '\t', len) : nullptr;
    out.name = (const char *)line; out.name_len = t ? (size_t)(t - line) : len;
    out.has_calls = t != nullptr;
    out.calls = t ? t + 1 : line + len; out.calls_len = t ? (size_t)(line + len - (t + 1)) : 0;
    return 1;
}

int host_rtab_pack(const uint8_t *calls, size_t len, bool has_calls, const int32_t *col2idx, int n_cols, uint32_t *present, uint32_t *missing, int row_words,
                   int32_t *n_present, int32_t *n_missing)
{
    *n_present = 0; *n_missing = 0;
    if (!has_calls) return NO_CALLS;
    const uint8_t *const e = calls + len;
    int64_t n_calls = 1;
    for (const uint8_t *p = calls; (p = (const uint8_t *)memchr(p, '\t', (size_t)(e - p))) != nullptr; ++p) ++n_calls;
    if (n_calls != n_cols) return MISMATCH;
    const uint8_t *p = calls;
    bool binary = true;
    for (int col = 0; col < n_cols && binary; ++col) {
        const uint8_t *t = (const uint8_t *)memchr(p, '\t', (size_t)(e - p));
        const uint8_t *fe = t ? t : e;
        const size_t n = (size_t)(fe - p);
        const int idx = col2idx[col];
        if (n == 0 || (n == 1 && *p == '.')) { if (idx >= 0) missing[idx >> 5] |= 1u << (idx & 31); }
        else if (n == 1 && *p == '1') { if (idx >= 0) present[idx >> 5] |= 1u << (idx & 31); }
        else if (!(n == 1 && *p == '0')) binary = false;
        p = fe + 1;
    }
    if (!binary) {
        memset(present, 0, sizeof(uint32_t) * (size_t)row_words); memset(missing, 0, sizeof(uint32_t) * (size_t)row_words);
        return NOT_BINARY;
    }
    int np = 0, nm = 0;
    for (int i = 0; i < row_words; ++i) { missing[i] &= ~present[i]; np += __builtin_popcount(present[i]); nm += __builtin_popcount(missing[i]); }
    *n_present = np; *n_missing = nm;
    return OK;
}

}  // namespace shrtab
