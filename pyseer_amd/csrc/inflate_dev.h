// inflate_dev.h -- one raw-DEFLATE member (RFC 1951), decoded by code that compiles for the host and for the device: the core of the
// k-mer reader's device inflate (k_bgzf_inflate, inflate_kernels.hip) and its host restatement (sh_inflate_host; a reader opened without a
// context; tools/inflate_core_check.cpp).  As with host_kmer_pack (kmer_kernels.h), the kernel's rule and the host's are the same text.
// inflate_fast.h stays the decoder of every other route and of the fallback.
//
// A BGZF member announces its compressed and its decoded size, and both are at most 64 KB.  shi_inflate decodes [cdata, cdata + clen) into
// [out, out + isize): stored, fixed and dynamic blocks, any number of them.  It reads no byte outside the first range and writes none
// outside the second, whatever the input holds, and every malformed input ends in one of the statuses below.  What zlib (the yardstick of
// tests/test_inflate_cpu.py) accepts is accepted, what it refuses is refused: an incomplete code only where its longest code has one bit,
// no more than 286 literal/length and 30 distance codes.
//
// The tables live in a ShInfTables the caller provides (LDS on the device), never in arrays of the thread's own.  Codes of up to
// SHI_LBITS / SHI_DBITS bits are looked up in one step (entry = symbol | length << 9, 0 = none); longer ones, and bit patterns that are no
// code of an incomplete set, are walked canonically, one bit per step, through count[] and symbol[].
//
// `W` says who runs the text.  On the host one thread does (ShInfOne).  On the device all 64 lanes of a wavefront run it on the same values
// (ShInfWave in inflate_kernels.hip): every lane decodes every symbol, lane 0 alone stores what is stored once (table entries, literals), and
// the loops that have a byte or an entry per step -- clearing a table, copying a stored block, copying a match -- are shared out over the
// lanes.  LDS operations of one wavefront complete in the order they were issued; W::sync() keeps the compiler from moving a lane's loads
// over another lane's stores: there is one between every store of lane 0 and the next read of that place by the other lanes, inside the
// loops of shi_build too, where each step reads the counters the step before it stored.
#pragma once
#include <stdint.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define SHI_HD __host__ __device__
#else
#define SHI_HD
#endif

enum ShInfStatus {
    SHI_OK = 0,
    SHI_BTYPE = 1,          // block type 3
    SHI_STORED_LEN = 2,     // stored block: LEN != ~NLEN
    SHI_OVERSUBSCRIBED = 3, // a set of code lengths that claims more than the code space
    SHI_INCOMPLETE = 4,     // a set that leaves code space unused (other than one code of one bit; no distance code at all is allowed too)
    SHI_REPEAT = 5,         // a repeat code with nothing to repeat, or running past HLIT + HDIST
    SHI_NO_EOB = 6,         // a dynamic block without an end-of-block code
    SHI_SYMBOL = 7,         // literal/length symbol 286 or 287, distance symbol 30 or 31
    SHI_DISTANCE = 8,       // a distance that reaches before the member's first byte
    SHI_INPUT_END = 9,      // the input ends inside a header, a symbol or a stored block
    SHI_OUTPUT_FULL = 10,   // more than isize bytes
    SHI_SHORT = 11,         // the final block ended with fewer than isize bytes
    SHI_COUNTS = 12,        // HLIT > 286 or HDIST > 30
    SHI_CODE = 13           // a bit pattern that is no code of an incomplete set
};

#define SHI_LBITS 10
#define SHI_DBITS 8
#define SHI_MEMBER_MAX 65536u

struct ShInfTables {
    uint16_t lfast[1 << SHI_LBITS], dfast[1 << SHI_DBITS];      // (dfast also serves the code-length code of a dynamic block's header)
    uint16_t lsym[288], dsym[32];
    uint16_t lcnt[16], dcnt[16];
    uint16_t offs[16], next[16];                                // shi_build's own
    uint8_t lens[320];                                          // HLIT + HDIST code lengths (fixed block: 288 and, from 288 on, 32)
    uint8_t clens[32];                                          // the 19 lengths of the code-length code
};

struct ShInfOne {
    SHI_HD uint32_t lane() const { return 0; }
    SHI_HD uint32_t width() const { return 1; }
    SHI_HD void sync() const {}
};

struct ShInfBits { const uint8_t *in; uint32_t len, pos; uint64_t bb; uint32_t bc; };        // bytes [0, pos) are consumed or among the bc bits of bb

static inline SHI_HD void shi_refill(ShInfBits &b)
{
    if (b.pos + 8 <= b.len) {
        // eight bytes at once; those that do not fit whole are taken again next time (their bits above bc are the stream's own)
        uint64_t v;
        __builtin_memcpy(&v, b.in + b.pos, 8);
        b.bb |= v << b.bc;
        const uint32_t adv = (63 - b.bc) >> 3;
        b.pos += adv; b.bc += adv * 8;
        return;
    }
    if (b.bc < 64) b.bb &= (1ull << b.bc) - 1;                  // (the last bytes: nothing above bc from here on)
    while (b.bc <= 56 && b.pos < b.len) { b.bb |= (uint64_t)b.in[b.pos++] << b.bc; b.bc += 8; }
}
static inline SHI_HD bool shi_need(ShInfBits &b, uint32_t n) { if (b.bc < n) shi_refill(b); return b.bc >= n; }                 // n <= 32
static inline SHI_HD uint32_t shi_take(ShInfBits &b, uint32_t n) { const uint32_t v = (uint32_t)b.bb & ((1u << n) - 1); b.bb >>= n; b.bc -= n; return v; }   // n <= 16

static inline SHI_HD uint32_t shi_reverse(uint32_t code, uint32_t len)
{
    uint32_t r = 0;
    for (uint32_t i = 0; i < len; ++i) { r = (r << 1) | (code & 1); code >>= 1; }
    return r;
}

// The decoding tables of `n` code lengths.  one_bit_ok: an incomplete set whose longest code has one bit passes, and so does an empty set.
template <class W>
static inline SHI_HD int shi_build(const uint8_t *lens, uint32_t n, uint16_t *cnt, uint16_t *sym, uint16_t *fast, uint32_t fbits, bool one_bit_ok,
                                   ShInfTables *t, const W &w)
{
    const bool me = w.lane() == 0;
    w.sync();
    for (uint32_t k = w.lane(); k < (1u << fbits); k += w.width()) fast[k] = 0;
    if (me) for (uint32_t l = 0; l < 16; ++l) cnt[l] = 0;
    w.sync();
    for (uint32_t i = 0; i < n; ++i) { const uint32_t l = lens[i]; const uint16_t c = cnt[l]; if (me) cnt[l] = (uint16_t)(c + 1); w.sync(); }
    int left = 1; uint32_t maxl = 0;
    for (uint32_t l = 1; l < 16; ++l) {
        left = left * 2 - (int)cnt[l];
        if (left < 0) return SHI_OVERSUBSCRIBED;
        if (cnt[l]) maxl = l;
    }
    if (left > 0 && !(one_bit_ok && maxl <= 1)) return SHI_INCOMPLETE;
    // where the symbols of a length begin in sym[], and the first code of a length
    uint32_t o = 0, code = 0;
    for (uint32_t l = 1; l < 16; ++l) {
        if (me) { t->offs[l] = (uint16_t)o; t->next[l] = (uint16_t)code; }
        o += cnt[l]; code = (code + cnt[l]) << 1;
    }
    w.sync();
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t l = lens[i];
        if (!l) continue;
        const uint32_t at = t->offs[l], c = t->next[l];
        if (me) { sym[at] = (uint16_t)i; t->offs[l] = (uint16_t)(at + 1); t->next[l] = (uint16_t)(c + 1); }
        if (l <= fbits) {
            const uint16_t e = (uint16_t)(i | (l << 9));
            for (uint32_t k = shi_reverse(c, l) + (w.lane() << l); k < (1u << fbits); k += w.width() << l) fast[k] = e;
        }
        w.sync();                                         // (the next step reads offs[] and next[])
    }
    return SHI_OK;
}

// the next symbol of the code (cnt, sym, fast), or minus a status
static inline SHI_HD int shi_symbol(ShInfBits &b, const uint16_t *fast, uint32_t fbits, const uint16_t *cnt, const uint16_t *sym)
{
    if (b.bc < 15) shi_refill(b);
    const uint32_t e = fast[(uint32_t)b.bb & ((1u << fbits) - 1)];
    if (e) {
        const uint32_t l = e >> 9;
        if (l > b.bc) return -SHI_INPUT_END;          // (no shorter code fits the bits that are left: it would have been found here)
        b.bb >>= l; b.bc -= l;
        return (int)(e & 511);
    }
    uint32_t code = 0, first = 0, index = 0;
    uint64_t bits = b.bb;
    for (uint32_t l = 1; l < 16; ++l) {
        if (l > b.bc) return -SHI_INPUT_END;
        code |= (uint32_t)bits & 1; bits >>= 1;
        const uint32_t count = cnt[l];
        if (code < first + count) { b.bb >>= l; b.bc -= l; return (int)sym[index + (code - first)]; }
        index += count; first = (first + count) << 1; code <<= 1;
    }
    return -SHI_CODE;
}

template <class W>
static inline SHI_HD int shi_inflate(const uint8_t *cdata, uint32_t clen, uint8_t *out, uint32_t isize, ShInfTables *t, uint32_t *produced, const W &w)
{
    const bool me = w.lane() == 0;
    ShInfBits b{cdata, clen, 0, 0, 0};
    uint32_t op = 0;
    int st = SHI_OK;
    for (;;) {
        if (!shi_need(b, 3)) { st = SHI_INPUT_END; break; }
        const uint32_t last = shi_take(b, 1), type = shi_take(b, 2);
        if (type == 3) { st = SHI_BTYPE; break; }
        if (type == 0) {
            // the rest of the byte is dropped, the whole bytes in hand go back
            b.bc &= ~7u;
            b.pos -= b.bc >> 3; b.bb = 0; b.bc = 0;
            if (clen - b.pos < 4) { st = SHI_INPUT_END; break; }
            const uint32_t len = (uint32_t)cdata[b.pos] | ((uint32_t)cdata[b.pos + 1] << 8), nlen = (uint32_t)cdata[b.pos + 2] | ((uint32_t)cdata[b.pos + 3] << 8);
            b.pos += 4;
            if ((len ^ 0xffffu) != nlen) { st = SHI_STORED_LEN; break; }
            if (len > clen - b.pos) { st = SHI_INPUT_END; break; }
            if (len > isize - op) { st = SHI_OUTPUT_FULL; break; }
            for (uint32_t i = w.lane(); i < len; i += w.width()) out[op + i] = cdata[b.pos + i];
            w.sync();
            op += len; b.pos += len;
        } else {
            uint32_t hlit = 288, hdist = 32;
            if (type == 1) {
                for (uint32_t i = w.lane(); i < 320; i += w.width()) t->lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
            } else {
                if (!shi_need(b, 14)) { st = SHI_INPUT_END; break; }
                hlit = shi_take(b, 5) + 257; hdist = shi_take(b, 5) + 1;
                const uint32_t hclen = shi_take(b, 4) + 4;
                if (hlit > 286 || hdist > 30) { st = SHI_COUNTS; break; }
                w.sync();
                for (uint32_t i = w.lane(); i < 19; i += w.width()) t->clens[i] = 0;
                w.sync();
                // the order of the code-length code's lengths (RFC 1951 3.2.7), five bits each
                const uint64_t order_lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
                const uint64_t order_hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
                for (uint32_t i = 0; i < hclen && !st; ++i) {
                    if (!shi_need(b, 3)) { st = SHI_INPUT_END; break; }
                    const uint32_t v = shi_take(b, 3), at = (uint32_t)((i < 12 ? order_lo >> (5 * i) : order_hi >> (5 * (i - 12))) & 31);
                    if (me) t->clens[at] = (uint8_t)v;
                }
                if (st) break;
                st = shi_build(t->clens, 19, t->dcnt, t->dsym, t->dfast, 7, false, t, w);
                if (st) break;
                const uint32_t total = hlit + hdist;
                uint32_t i = 0;
                while (i < total) {
                    const int s = shi_symbol(b, t->dfast, 7, t->dcnt, t->dsym);
                    if (s < 0) { st = -s; break; }
                    if (s < 16) { if (me) t->lens[i] = (uint8_t)s; w.sync(); ++i; continue; }
                    uint32_t prev = 0, rep;
                    if (s == 16) {
                        if (i == 0) { st = SHI_REPEAT; break; }
                        prev = t->lens[i - 1];
                        if (!shi_need(b, 2)) { st = SHI_INPUT_END; break; }
                        rep = 3 + shi_take(b, 2);
                    } else if (s == 17) {
                        if (!shi_need(b, 3)) { st = SHI_INPUT_END; break; }
                        rep = 3 + shi_take(b, 3);
                    } else {
                        if (!shi_need(b, 7)) { st = SHI_INPUT_END; break; }
                        rep = 11 + shi_take(b, 7);
                    }
                    if (i + rep > total) { st = SHI_REPEAT; break; }
                    for (uint32_t k = w.lane(); k < rep; k += w.width()) t->lens[i + k] = (uint8_t)prev;
                    w.sync();
                    i += rep;
                }
                if (st) break;
                if (t->lens[256] == 0) { st = SHI_NO_EOB; break; }
            }
            w.sync();
            st = shi_build(t->lens, hlit, t->lcnt, t->lsym, t->lfast, SHI_LBITS, true, t, w);
            if (st) break;
            st = shi_build(t->lens + hlit, hdist, t->dcnt, t->dsym, t->dfast, SHI_DBITS, true, t, w);
            if (st) break;
            for (;;) {
                int s = shi_symbol(b, t->lfast, SHI_LBITS, t->lcnt, t->lsym);
                if (s < 0) { st = -s; break; }
                if (s < 256) {
                    if (op >= isize) { st = SHI_OUTPUT_FULL; break; }
                    if (me) out[op] = (uint8_t)s;
                    ++op;
                    continue;
                }
                if (s == 256) break;
                if (s >= 286) { st = SHI_SYMBOL; break; }
                // lengths 3 .. 258 from symbols 257 .. 285, distances 1 .. 32768 from symbols 0 .. 29 (RFC 1951 3.2.5), computed
                s -= 257;
                uint32_t len = 258;
                if (s < 8) len = 3 + (uint32_t)s;
                else if (s < 28) {
                    const uint32_t x = ((uint32_t)s >> 2) - 1;
                    if (!shi_need(b, x)) { st = SHI_INPUT_END; break; }
                    len = 3 + ((4 + ((uint32_t)s & 3)) << x) + shi_take(b, x);
                }
                const int d = shi_symbol(b, t->dfast, SHI_DBITS, t->dcnt, t->dsym);
                if (d < 0) { st = -d; break; }
                if (d >= 30) { st = SHI_SYMBOL; break; }
                uint32_t dist = 1 + (uint32_t)d;
                if (d >= 4) {
                    const uint32_t x = ((uint32_t)d >> 1) - 1;
                    if (!shi_need(b, x)) { st = SHI_INPUT_END; break; }
                    dist = 1 + ((2 + ((uint32_t)d & 1)) << x) + shi_take(b, x);
                }
                if (dist > op) { st = SHI_DISTANCE; break; }
                if (len > isize - op) { st = SHI_OUTPUT_FULL; break; }
                // byte i of the match is byte i mod dist of the dist bytes before it: every source lies before op, so the lanes need no order
                w.sync();
                const uint8_t *src = out + (op - dist);
                for (uint32_t i = w.lane(); i < len; i += w.width()) out[op + i] = src[i < dist ? i : i % dist];
                w.sync();
                op += len;
            }
            if (st) break;
        }
        if (last) break;
    }
    if (!st && op != isize) st = SHI_SHORT;
    *produced = op;
    return st;
}

// the table of a batch of members for k_bgzf_inflate: where the compressed bytes lie, and where the text goes
struct ShInfMember {
    uint64_t coff, ooff;       // of cdata from the start of the compressed buffer, of the text from the start of the output buffer
    uint32_t clen, isize;
};

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
size_t shk_bgzf_inflate_lds_bytes();
// one wavefront per member: text[ooff .. ooff + min(produced, isize)) is written and nothing else; status[i], produced[i]
hipError_t shk_bgzf_inflate(hipStream_t st, const uint8_t *comp, const ShInfMember *mem, int64_t n, uint8_t *text, int32_t *status, uint32_t *produced);
#endif
