// vcf_reader.cpp -- native VCF text reader, host half: the reference reads VCF through pysam (pyseer/input.py:455-503) and uses the contig,
// the position, the alleles, FILTER and every sample's GT.  All of that is in the tab-separated line, so this reader needs no htslib:
//   * the container: plain text, gzip (inflate_fast.h, one thread: the format is sequential) or BGZF -- what `bgzip` writes and tabix wants
//     -- whose members are independent and announce their size, decoded by a pool of threads; CRC-32 of every member checked;
//   * framing into lines (a last line without newline, \r\n, a line longer than the window: the window grows);
//   * the header: `#CHROM ...` -> column -> index in the phenotype's sample list, or -1;
//   * the nine fixed columns of a record: the name CHROM_POS_REF[_ALT], the skip reason (more than one ALT; a FILTER that is neither empty
//     nor holds PASS), POS, len(REF) (the span burden regions are matched against), where GT sits in FORMAT.
// The sample columns -- ~99 % of the bytes: `0:186,0:186:99:0,1800` per sample -- are NOT tokenised here: next() hands them out as they
// stand, and csrc/vcf_api.inc sends them to the device (k_vcf_gt_pack, csrc/vcf_kernels.hip).  No index file (.tbi / .csi) is read.
// BCF 2.1 / 2.2 (the section "BCF" below) comes through the same container and window: the format is sniffed from the first decoded bytes,
// records are framed by their two length words, the shared block gives what the nine columns give, and of the individual block only the GT
// vector is handed out -- n_sample x L typed integers, which k_bcf_gt_pack reduces on the device.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstring>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "crc32_clmul.h"
#include "host_pool.h"
#include "inflate_fast.h"
#include "vcf_reader.h"

namespace shvcf {

static const size_t FILL = 8u << 20;                     // text decoded per refill
static const size_t HIST = 32768;                        // DEFLATE history kept in front of the unread text

// BGZF member at p: total compressed size, or 0 if p is not a BGZF member header (RFC 1952 extra field 'BC')
static size_t bgzf_member(const uint8_t *p, const uint8_t *end)
{
    if (end - p < 18 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || !(p[3] & 4)) return 0;
    const int xlen = p[10] | (p[11] << 8);
    const uint8_t *x = p + 12, *xe = x + xlen;
    if (xe > end) return 0;
    while (x + 4 <= xe) {
        const int slen = x[2] | (x[3] << 8);
        if (x[0] == 'B' && x[1] == 'C' && slen == 2 && x + 6 <= xe) return (size_t)(x[4] | (x[5] << 8)) + 1;
        x += 4 + slen;
    }
    return 0;
}

struct Reader {
    int fd = -1; const uint8_t *map = nullptr; size_t map_len = 0; int mode = 0;
    // the window of decoded text: [beg, end) is unread, [scan, end) has not been searched for a newline yet
    std::vector<uint8_t> win; size_t beg = 0, scan = 0, end = 0; bool eof = false;
    size_t ppos = 0;                                      // plain / BGZF: next compressed byte
    shinf::Decoder dec; uint32_t crc_run = 0;             // gzip
    std::unique_ptr<shost::ParPool> pool;                 // BGZF
    // header
    std::vector<int32_t> col2idx; bool have_header = false;
    std::unordered_map<std::string, int> contig_id; std::vector<std::string> contigs;
    std::unordered_map<std::string, int> sample_idx;
    std::string name;
    // BCF: 1 if the decoded stream is BCF2; records read so far; the dictionary index of GT (-1: not declared); index -> contig name
    int format = 0; int64_t bcf_rec = 0; int bcf_gt_key = -1; std::unordered_map<int64_t, std::string> bcf_contigs;
    std::vector<uint8_t> narrow;                          // a GT vector of int16 / int32 values in the int8 coding
    ~Reader() { if (map && map_len) munmap((void *)map, map_len); if (fd >= 0) ::close(fd); }
};

// room for at least FILL more bytes behind `end`: drop what has been read (but HIST bytes of it), then grow
static void make_room(Reader *r)
{
    if (r->win.size() - r->end >= FILL + 512) return;
    const size_t keep = r->beg > HIST ? r->beg - HIST : 0;
    if (keep) { memmove(r->win.data(), r->win.data() + keep, r->end - keep); r->beg -= keep; r->scan -= keep; r->end -= keep; }
    if (r->win.size() - r->end < FILL + 512) r->win.resize(r->end + FILL + 512);
}

// appends text to the window; false at the end of the file or on error (err set)
static bool fill(Reader *r, std::string &err)
{
    if (r->eof) return false;
    make_room(r);
    uint8_t *const base = r->win.data();
    if (r->mode == 0) {
        const size_t n = std::min(FILL, r->map_len - r->ppos);
        memcpy(base + r->end, r->map + r->ppos, n); r->ppos += n; r->end += n;
        if (r->ppos >= r->map_len) r->eof = true;
        return n > 0;
    }
    if (r->mode == 1) {
        shinf::Decoder &d = r->dec;
        uint8_t *const start = base + r->end, *out = start, *const lim = start + FILL + 512;
        const uint8_t *crc_from = start;
        for (;;) {
            uint8_t *const before = out;
            out = d.run(out, lim, base);
            for (int i = 0; i < d.n_ends; ++i) {          // members that ended in this stretch: their CRC-32
                r->crc_run = shcrc::crc32(r->crc_run, crc_from, (size_t)(d.ends[i].at - crc_from));
                if (r->crc_run != d.ends[i].crc) { err = "gzip: CRC-32 check failed"; r->eof = true; return false; }
                r->crc_run = 0; crc_from = d.ends[i].at;
            }
            const bool full = d.n_ends == 64;
            d.n_ends = 0;
            if (d.state == shinf::Decoder::ERROR) { err = std::string("gzip: ") + (d.err ? d.err : "error"); r->eof = true; return false; }
            if (d.state == shinf::Decoder::DONE) { r->eof = true; break; }
            if ((size_t)(lim - out) < 300) break;
            if (out == before && !full) { err = "gzip: truncated stream"; r->eof = true; return false; }
        }
        r->crc_run = shcrc::crc32(r->crc_run, crc_from, (size_t)(out - crc_from));
        r->end += (size_t)(out - start);
        return out > start;
    }
    // BGZF: as many members as fit, decoded side by side
    struct Mem { const uint8_t *cdata; size_t clen; uint32_t isize, crc; size_t off; };
    std::vector<Mem> mem;
    size_t total = 0;
    const uint8_t *p = r->map + r->ppos, *const fend = r->map + r->map_len;
    while (p < fend && total + 65536 <= FILL) {
        const size_t bs = bgzf_member(p, fend);
        if (bs < 26 || p + bs > fend) { err = "BGZF: bad member header"; r->eof = true; return false; }
        const int xlen = p[10] | (p[11] << 8);
        const uint8_t *cd = p + 12 + xlen, *tr = p + bs - 8;
        if (cd > tr) { err = "BGZF: bad member header"; r->eof = true; return false; }
        Mem m{cd, (size_t)(tr - cd), (uint32_t)tr[4] | ((uint32_t)tr[5] << 8) | ((uint32_t)tr[6] << 16) | ((uint32_t)tr[7] << 24),
              (uint32_t)tr[0] | ((uint32_t)tr[1] << 8) | ((uint32_t)tr[2] << 16) | ((uint32_t)tr[3] << 24), total};
        if (m.isize > 65536) { err = "BGZF: member larger than 64 KB"; r->eof = true; return false; }
        total += m.isize; mem.push_back(m); p += bs;
    }
    r->ppos = (size_t)(p - r->map);
    if (p >= fend) r->eof = true;
    std::atomic<int> bad{0};
    uint8_t *const dst = base + r->end;
    r->pool->run((int64_t)mem.size(), 4, [&](int64_t i) {
        static thread_local std::vector<uint8_t> tmp(65536 + 512);
        static thread_local shinf::Decoder d;
        const Mem &m = mem[(size_t)i];
        d.begin(m.cdata, m.cdata + m.clen, true);
        uint8_t *o = d.run(tmp.data(), tmp.data() + tmp.size(), tmp.data());
        if (d.state != shinf::Decoder::DONE || (size_t)(o - tmp.data()) != m.isize || shcrc::crc32(0u, tmp.data(), m.isize) != m.crc) ++bad;
        else memcpy(dst + m.off, tmp.data(), m.isize);
    });
    if (bad) { err = "BGZF: a member failed to decode or its CRC-32 check"; r->eof = true; return false; }
    r->end += total;
    return total > 0 || !r->eof;
}

// the next line without its terminator; false at the end of the text (or on error: err set)
static bool next_line(Reader *r, const uint8_t *&line, size_t &len, std::string &err)
{
    for (;;) {
        if (const void *nl = r->scan < r->end ? memchr(r->win.data() + r->scan, '\n', r->end - r->scan) : nullptr) {
            const size_t at = (size_t)((const uint8_t *)nl - r->win.data());
            line = r->win.data() + r->beg; len = at - r->beg;
            r->beg = r->scan = at + 1;
            break;
        }
        r->scan = r->end;
        if (r->eof) {
            if (r->beg >= r->end) return false;
            line = r->win.data() + r->beg; len = r->end - r->beg;          // a last line without newline
            r->beg = r->scan = r->end;
            break;
        }
        if (!fill(r, err) && !err.empty()) return false;
    }
    if (len && line[len - 1] == '\r') --len;
    return true;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// BCF 2.1 / 2.2.  All integers little-endian.  File: "BCF" 2 minor | l_text u32 | header text (VCF header, NUL-terminated) | records.
// Record: l_shared u32 | l_indiv u32 | shared: CHROM i32, POS i32 (0-based), rlen i32, QUAL f32, n_allele<<16|n_info u32, n_fmt<<24|n_sample
// u32, ID, n_allele alleles (typed strings), FILTER (typed ints), INFO (not read) | individual: n_fmt x (key typed int, descriptor with the
// per-sample count L, n_sample x L values).  A typed value starts with a descriptor byte: low 4 bits the type (0 void, 1 int8, 2 int16,
// 3 int32, 5 float32, 7 char), high 4 bits the count, 15 = a typed integer with the count follows.
// ---------------------------------------------------------------------------------------------------------------------------------------

// at least n unread bytes in the window; false when the stream ends before (or on error: err set)
static bool ensure(Reader *r, size_t n, std::string &err)
{
    while (r->end - r->beg < n)
        if (!fill(r, err)) return r->end - r->beg >= n;
    return true;
}

static inline uint32_t le32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// ID and IDX of a `##KIND=<key=value,...>` line (values may be quoted); p: behind '<'.  false: the line has no ID
static bool meta_id(const char *p, const char *const e, std::string &id, int64_t &idx)
{
    bool have = false;
    idx = -1;
    while (p < e && *p != '>') {
        const char *k = p;
        while (p < e && *p != '=' && *p != ',' && *p != '>') ++p;
        const std::string key(k, p);
        std::string val;
        if (p < e && *p == '=') {
            ++p;
            if (p < e && *p == '"') {
                ++p;
                while (p < e && *p != '"') { if (*p == '\\' && p + 1 < e) ++p; val += *p++; }
                if (p < e) ++p;
            } else {
                const char *v = p;
                while (p < e && *p != ',' && *p != '>') ++p;
                val.assign(v, p);
            }
        }
        if (key == "ID") { id = val; have = true; }
        else if (key == "IDX") { idx = -1; if (!val.empty() && val.size() < 10 && val.find_first_not_of("0123456789") == std::string::npos) idx = atoll(val.c_str()); }
        if (p < e && *p == ',') ++p;
    }
    return have;
}

// the file head behind the sniffed "BCF": version, header text -> the dictionary's GT, the contigs, the sample columns
static bool bcf_head(Reader *r, const char *path, std::string &err)
{
    if (!ensure(r, 9, err)) { if (err.empty()) err = std::string(path) + ": BCF: the file ends inside its head"; return false; }
    const uint8_t *h = r->win.data() + r->beg;
    if (h[3] == 4) { err = std::string(path) + " is BCF1 (BCF\\4), which is not read: BCF 2.1 and 2.2 are"; return false; }
    if (h[3] != 2) { err = std::string(path) + ": BCF major version " + std::to_string((int)h[3]) + " is not read: BCF 2.1 and 2.2 are"; return false; }
    if (h[4] != 1 && h[4] != 2) { err = std::string(path) + ": BCF minor version " + std::to_string((int)h[4]) + " is not read: BCF 2.1 and 2.2 are"; return false; }
    const size_t l_text = le32(h + 5);
    if (!ensure(r, 9 + l_text, err)) { if (err.empty()) err = std::string(path) + ": BCF: the file ends inside its header text"; return false; }
    const char *t = (const char *)r->win.data() + r->beg + 9, *const te = t + l_text;
    const char *const nul = (const char *)memchr(t, 0, l_text), *const end = nul ? nul : te;
    std::unordered_map<std::string, int64_t> dict;
    dict.emplace("PASS", 0);
    int64_t n_contig = 0;
    std::string id;
    while (t < end) {
        const char *nl = (const char *)memchr(t, '\n', (size_t)(end - t));
        const char *le = nl ? nl : end;
        const char *const next_t = nl ? nl + 1 : end;
        if (le > t && le[-1] == '\r') --le;
        const size_t len = (size_t)(le - t);
        int64_t idx;
        if (len >= 10 && memcmp(t, "##contig=<", 10) == 0) {
            if (meta_id(t + 10, le, id, idx)) { r->bcf_contigs.emplace(idx >= 0 ? idx : n_contig, id); ++n_contig; }
        } else if ((len >= 10 && memcmp(t, "##FILTER=<", 10) == 0) || (len >= 10 && memcmp(t, "##FORMAT=<", 10) == 0) || (len >= 8 && memcmp(t, "##INFO=<", 8) == 0)) {
            if (meta_id(t + (t[2] == 'I' ? 8 : 10), le, id, idx) && !dict.count(id)) { const int64_t at = idx >= 0 ? idx : (int64_t)dict.size(); dict.emplace(id, at); }
        } else if (len >= 6 && memcmp(t, "#CHROM", 6) == 0) {
            int col = 0;
            for (const char *p = t; p <= le;) {
                const char *tab = (const char *)memchr(p, '\t', (size_t)(le - p));
                if (!tab) tab = le;
                if (col >= 9) {
                    auto it = r->sample_idx.find(std::string(p, (size_t)(tab - p)));
                    r->col2idx.push_back(it == r->sample_idx.end() ? -1 : it->second);
                }
                ++col; p = tab + 1;
            }
            r->have_header = true;
        }
        t = next_t;
    }
    if (!r->have_header) { err = std::string(path) + ": the BCF header text has no #CHROM line"; return false; }
    auto gt = dict.find("GT");
    r->bcf_gt_key = gt == dict.end() ? -1 : (int)gt->second;
    r->beg += 9 + l_text; r->scan = r->beg;
    r->format = 1;
    return true;
}

struct Cur { const uint8_t *p, *e; };

// a typed integer scalar (the count in a long descriptor; a FORMAT key)
static bool typed_scalar(Cur &c, int64_t &v)
{
    if (c.p >= c.e) return false;
    const uint8_t d = *c.p++;
    const int t = d & 15;
    if ((d >> 4) != 1 || t < 1 || t > 3) return false;
    const size_t w = (size_t)1 << (t - 1);
    if ((size_t)(c.e - c.p) < w) return false;
    v = t == 1 ? (int64_t)(int8_t)c.p[0] : t == 2 ? (int64_t)(int16_t)(c.p[0] | (c.p[1] << 8)) : (int64_t)(int32_t)le32(c.p);
    c.p += w;
    return true;
}

static bool typed_desc(Cur &c, int &type, uint64_t &count)
{
    if (c.p >= c.e) return false;
    const uint8_t d = *c.p++;
    type = d & 15; count = d >> 4;
    if (count == 15) { int64_t v; if (!typed_scalar(c, v) || v < 0) return false; count = (uint64_t)v; }
    return true;
}

static inline size_t type_width(int type) { return type == 1 || type == 7 ? 1 : type == 2 ? 2 : type == 3 || type == 5 ? 4 : 0; }

static bool typed_string(Cur &c, const uint8_t *&s, size_t &n)
{
    int type; uint64_t count;
    if (!typed_desc(c, type, count)) return false;
    if (type == 0) { s = c.p; n = 0; return true; }
    if (type != 7 || (uint64_t)(c.e - c.p) < count) return false;
    s = c.p; n = (size_t)count; c.p += count;
    return true;
}

// int16 / int32 GT values in the int8 coding: the end-of-vector and the missing mark become int8's, an allele index int8 cannot hold (a kept
// record has at most two alleles: none of its values needs more) stays a non-zero allele
static void narrow_gt(uint8_t *dst, const uint8_t *src, size_t n, int width)
{
    for (size_t i = 0; i < n; ++i) {
        const uint32_t v = width == 2 ? (uint32_t)(src[2 * i] | (src[2 * i + 1] << 8)) : le32(src + 4 * i);
        const uint32_t eov = width == 2 ? 0x8001u : 0x80000001u, mis = width == 2 ? 0x8000u : 0x80000000u;
        dst[i] = v == eov ? 0x81 : v == mis ? 0x80 : v < 0x80u ? (uint8_t)v : (uint8_t)(0x7e | (v & 1u));
    }
}

static int bcf_next(Reader *r, Record &rec, std::string &err)
{
    if (!ensure(r, 8, err)) {
        if (!err.empty()) return -1;
        if (r->end == r->beg) return 0;
        err = "BCF: the file ends inside the lengths of record " + std::to_string(r->bcf_rec + 1); return -1;
    }
    const int64_t no = ++r->bcf_rec;
    const std::string where = "BCF: record " + std::to_string(no) + ": ";
    const size_t l_shared = le32(r->win.data() + r->beg), l_indiv = le32(r->win.data() + r->beg + 4);
    if (!ensure(r, 8 + l_shared + l_indiv, err)) { if (err.empty()) err = where + "the file ends inside it"; return -1; }
    const uint8_t *const sh = r->win.data() + r->beg + 8;
    r->beg += 8 + l_shared + l_indiv; r->scan = r->beg;
    if (l_shared < 24) { err = where + "a shared block shorter than its fixed part"; return -1; }
    const int64_t chrom = (int32_t)le32(sh), pos0 = (int32_t)le32(sh + 4);
    const uint32_t n_allele = le32(sh + 16) >> 16, n_fmt = le32(sh + 20) >> 24, n_sample = le32(sh + 20) & 0xffffffu;
    auto ct = r->bcf_contigs.find(chrom);
    if (ct == r->bcf_contigs.end()) { err = where + "CHROM index " + std::to_string(chrom) + " names no ##contig line of the header"; return -1; }
    if (n_sample != 0 && n_sample != (uint32_t)r->col2idx.size()) {
        err = where + "n_sample is " + std::to_string(n_sample) + ", the header has " + std::to_string(r->col2idx.size()) + " sample columns"; return -1;
    }
    Cur c{sh + 24, sh + l_shared};
    const uint8_t *s; size_t n;
    if (!typed_string(c, s, n)) { err = where + "ID runs past the shared block"; return -1; }
    const std::string &chrom_name = ct->second;
    auto it = r->contig_id.find(chrom_name);
    if (it == r->contig_id.end()) { it = r->contig_id.emplace(chrom_name, (int)r->contigs.size()).first; r->contigs.push_back(chrom_name); }
    rec.contig = it->second;
    rec.pos = pos0 + 1;
    rec.ref_len = 0;
    r->name.assign(chrom_name); r->name += '_'; r->name += std::to_string(pos0 + 1); r->name += '_';
    for (uint32_t a = 0; a < n_allele; ++a) {
        if (!typed_string(c, s, n)) { err = where + "an allele runs past the shared block"; return -1; }
        if (a == 0) rec.ref_len = (int32_t)n;
        if (a) r->name += a == 1 ? '_' : ',';              // (several ALTs: the text route's name carries ALT as it stands, commas included)
        r->name.append((const char *)s, n);
    }
    rec.name = r->name.data(); rec.name_len = r->name.size();
    int type; uint64_t count;
    if (!typed_desc(c, type, count) || (type != 0 && (type > 3 || (uint64_t)(c.e - c.p) < count * type_width(type)))) { err = where + "FILTER runs past the shared block"; return -1; }
    bool any = false, pass = false;
    if (type != 0)
        for (uint64_t i = 0; i < count; ++i) {
            const uint8_t *q = c.p + i * type_width(type);
            const uint32_t v = type == 1 ? q[0] : type == 2 ? (uint32_t)(q[0] | (q[1] << 8)) : le32(q);
            const uint32_t mis = type == 1 ? 0x80u : type == 2 ? 0x8000u : 0x80000000u;
            if (v == mis || v == mis + 1) continue;       // (a missing entry names no filter)
            any = true;
            if (v == 0) pass = true;
        }
    rec.skip = n_allele > 2 ? MULTI : ((any && !pass) ? FILTERED : KEPT);
    rec.gt = -1; rec.samp = sh + l_shared; rec.samp_len = 0;
    if (rec.skip != KEPT || n_sample == 0) return 1;
    // the individual block: every field before GT is skipped by its length
    Cur d{sh + l_shared, sh + l_shared + l_indiv};
    for (uint32_t f = 0; f < n_fmt; ++f) {
        int64_t key;
        if (!typed_scalar(d, key) || !typed_desc(d, type, count)) { err = where + "a FORMAT field runs past the individual block"; return -1; }
        const size_t w = type_width(type);
        if (type != 0 && w == 0) { err = where + "a FORMAT field of unknown type " + std::to_string(type); return -1; }
        if (count > (uint64_t)1 << 31 || (uint64_t)(d.e - d.p) < count * w * n_sample) { err = where + "a FORMAT field runs past the individual block"; return -1; }
        if (key == r->bcf_gt_key && r->bcf_gt_key >= 0) {
            if (type == 0 || count == 0) break;           // an empty vector: every sample missing
            if (type > 3) { err = where + "GT is not a vector of integers"; return -1; }
            const size_t vals = (size_t)count * n_sample;
            if (vals >= ((size_t)1 << 31)) { err = where + "a GT vector of 2 GB or more"; return -1; }
            rec.gt = (int32_t)count; rec.samp_len = vals;
            if (w == 1) rec.samp = d.p;
            else { r->narrow.resize(vals); narrow_gt(r->narrow.data(), d.p, vals, (int)w); rec.samp = r->narrow.data(); }   // (the rare path)
            break;
        }
        d.p += count * w * n_sample;
    }
    return 1;
}

Reader *open_file(const char *path, const char *const *sample_names, int n_samples, std::string &err)
{
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
    r->mode = (r->map_len >= 2 && r->map[0] == 0x1f && r->map[1] == 0x8b) ? (bgzf_member(r->map, r->map + r->map_len) ? 2 : 1) : 0;
    if (r->mode == 1) r->dec.begin(r->map, r->map + r->map_len);
    if (r->mode == 2) r->pool.reset(new shost::ParPool(std::max(1, std::min(16, shost::per_stream_cpus(2)) - 1), shost::ST_READER_DECODE));
    if (r->map_len == 0) r->eof = true;
    for (int i = 0; i < n_samples; ++i) r->sample_idx.emplace(sample_names[i], i);
    // BCF or text: the first decoded bytes tell ("BCF" + major version; a VCF starts with '#')
    if (!ensure(r.get(), 5, err) && !err.empty()) return nullptr;
    if (r->end - r->beg >= 4 && memcmp(r->win.data() + r->beg, "BCF", 3) == 0) {
        if (!bcf_head(r.get(), path, err)) return nullptr;
        return r.release();
    }
    // the header: everything up to and including the #CHROM line
    const uint8_t *line; size_t len;
    while (!r->have_header) {
        const size_t at = r->beg;
        if (!next_line(r.get(), line, len, err)) break;
        if (len == 0) continue;
        if (line[0] != '#') { r->beg = r->scan = at; break; }              // a record before any #CHROM line
        if (len >= 6 && memcmp(line, "#CHROM", 6) == 0) {
            int col = 0;
            const uint8_t *p = line, *const e = line + len;
            while (p <= e) {
                const uint8_t *t = (const uint8_t *)memchr(p, '\t', (size_t)(e - p));
                if (!t) t = e;
                if (col >= 9) {
                    auto it = r->sample_idx.find(std::string((const char *)p, (size_t)(t - p)));
                    r->col2idx.push_back(it == r->sample_idx.end() ? -1 : it->second);
                }
                ++col; p = t + 1;
            }
            r->have_header = true;
        }
    }
    if (!err.empty()) return nullptr;
    if (!r->have_header) { err = std::string(path) + " has no #CHROM header line; is this a VCF file?"; return nullptr; }
    return r.release();
}

void close_file(Reader *r) { delete r; }
int n_cols(const Reader *r) { return (int)r->col2idx.size(); }
const int32_t *col_to_sample(const Reader *r) { return r->col2idx.data(); }
int n_contigs(const Reader *r) { return (int)r->contigs.size(); }
const char *contig_name(const Reader *r, int id) { return id >= 0 && id < (int)r->contigs.size() ? r->contigs[(size_t)id].c_str() : ""; }
int mode(const Reader *r) { return r->mode; }
int format(const Reader *r) { return r->format; }

int next(Reader *r, Record &rec, std::string &err)
{
    if (r->format) return bcf_next(r, rec, err);
    const uint8_t *line; size_t len;
    do {
        if (!next_line(r, line, len, err)) return err.empty() ? 0 : -1;
    } while (len == 0 || line[0] == '#');
    // the nine fixed columns; a line that ends early leaves the rest empty
    const uint8_t *col[9]; size_t clen[9];
    const uint8_t *p = line, *const e = line + len;
    bool ended = false;
    for (int c = 0; c < 9; ++c) {
        if (ended) { col[c] = e; clen[c] = 0; continue; }
        col[c] = p;
        const uint8_t *t = (const uint8_t *)memchr(p, '\t', (size_t)(e - p));
        if (!t) { clen[c] = (size_t)(e - p); ended = true; } else { clen[c] = (size_t)(t - p); p = t + 1; }
    }
    const bool has_samples = !ended;
    rec.samp = has_samples ? p : e; rec.samp_len = has_samples ? (size_t)(e - p) : 0;
    const std::string chrom((const char *)col[0], clen[0]);
    auto it = r->contig_id.find(chrom);
    if (it == r->contig_id.end()) { it = r->contig_id.emplace(chrom, (int)r->contigs.size()).first; r->contigs.push_back(chrom); }
    rec.contig = it->second;
    rec.pos = 0;
    for (size_t i = 0; i < clen[1]; ++i) {
        if (col[1][i] < '0' || col[1][i] > '9') { err = "VCF: POS is not a number in the record at " + chrom + ":" + std::string((const char *)col[1], clen[1]); return -1; }
        rec.pos = rec.pos * 10 + (col[1][i] - '0');
    }
    if (clen[1] == 0) { err = "VCF: a record without POS"; return -1; }
    rec.ref_len = (int32_t)clen[3];
    const bool no_alt = clen[4] == 0 || (clen[4] == 1 && col[4][0] == '.');
    r->name.assign(chrom); r->name += '_'; r->name.append((const char *)col[1], clen[1]); r->name += '_'; r->name.append((const char *)col[3], clen[3]);
    if (!no_alt) { r->name += '_'; r->name.append((const char *)col[4], clen[4]); }
    rec.name = r->name.data(); rec.name_len = r->name.size();
    // FILTER: kept if it names no filter ('.' or empty entries do not count) or one of its entries is PASS
    bool any = false, pass = false;
    for (const uint8_t *q = col[6], *const qe = col[6] + clen[6]; q <= qe;) {
        const uint8_t *t = q < qe ? (const uint8_t *)memchr(q, ';', (size_t)(qe - q)) : nullptr;
        if (!t) t = qe;
        const size_t n = (size_t)(t - q);
        if (n && !(n == 1 && q[0] == '.')) { any = true; if (n == 4 && memcmp(q, "PASS", 4) == 0) pass = true; }
        q = t + 1;
    }
    rec.skip = memchr(col[4], ',', clen[4]) ? MULTI : ((any && !pass) ? FILTERED : KEPT);
    // where GT sits in FORMAT
    rec.gt = -1;
    int sub = 0;
    for (const uint8_t *q = col[8], *const qe = col[8] + clen[8]; q <= qe; ++sub) {
        const uint8_t *t = q < qe ? (const uint8_t *)memchr(q, ':', (size_t)(qe - q)) : nullptr;
        if (!t) t = qe;
        if (t - q == 2 && q[0] == 'G' && q[1] == 'T') { rec.gt = sub; break; }
        q = t + 1;
    }
    return 1;
}

static inline int gt_code(const uint8_t *p, const uint8_t *const e, const int gi)
{
    int colons = 0;
    while (colons < gi) {
        if (p >= e) return 2;
        const uint8_t c = *p++;
        if (c == ':') ++colons;
    }
    bool tok0 = false;
    for (; p < e; ++p) {
        const uint8_t c = *p;
        if (c == ':') break;
        if (c == '/' || c == '|') tok0 = false;
        else if (c >= '1' && c <= '9') return 1;
        else if (c == '0') tok0 = true;
    }
    return tok0 ? 0 : 2;
}

void host_gt_pack(const uint8_t *samp, size_t len, int gt, const int32_t *col2idx, int n_cols, uint32_t *present, uint32_t *missing, int row_words,
                  int32_t *n_present, int32_t *n_missing)
{
    int col = 0;
    if (gt >= 0) {
        const uint8_t *p = samp, *const e = samp + len;
        for (; col < n_cols; ++col) {
            const uint8_t *t = (const uint8_t *)memchr(p, '\t', (size_t)(e - p));
            const uint8_t *fe = t ? t : e;
            const int idx = col2idx[col];
            if (idx >= 0) {
                const int code = gt_code(p, fe, gt);
                if (code == 1) present[idx >> 5] |= 1u << (idx & 31);
                else if (code == 2) missing[idx >> 5] |= 1u << (idx & 31);
            }
            if (!t) { ++col; break; }
            p = t + 1;
        }
    }
    if (gt >= -1)
        for (; col < n_cols; ++col) { const int idx = col2idx[col]; if (idx >= 0) missing[idx >> 5] |= 1u << (idx & 31); }
    int np = 0, nm = 0;
    for (int i = 0; i < row_words; ++i) { missing[i] &= ~present[i]; np += __builtin_popcount(present[i]); nm += __builtin_popcount(missing[i]); }
    *n_present = np; *n_missing = nm;
}

// the three-way code of one sample's L GT values in the int8 coding (k_bcf_gt_pack's bcf_gt_code restated)
static inline int bcf_gt_code(const uint8_t *p, const uint32_t L)
{
    int last = 2;
    for (uint32_t j = 0; j < L; ++j) {
        const uint8_t b = p[j];
        if (b == 0x81) break;                             // end of vector
        if (b == 0x80) { last = 2; continue; }            // the type's missing value
        const int allele = (b >> 1) - 1;
        if (allele >= 1) return 1;
        last = allele == 0 ? 0 : 2;
    }
    return last;
}

void host_bcf_pack(const uint8_t *gt, uint32_t L, int has_gt, const int32_t *col2idx, int n_cols, uint32_t *present, uint32_t *missing, int row_words,
                   int32_t *n_present, int32_t *n_missing)
{
    if (has_gt >= -1)
        for (int col = 0; col < n_cols; ++col) {
            const int idx = col2idx[col];
            if (idx < 0) continue;
            const int code = has_gt >= 0 ? bcf_gt_code(gt + (size_t)col * L, L) : 2;
            if (code == 1) present[idx >> 5] |= 1u << (idx & 31);
            else if (code == 2) missing[idx >> 5] |= 1u << (idx & 31);
        }
    int np = 0, nm = 0;
    for (int i = 0; i < row_words; ++i) { missing[i] &= ~present[i]; np += __builtin_popcount(present[i]); nm += __builtin_popcount(missing[i]); }
    *n_present = np; *n_missing = nm;
}

}  // namespace shvcf
