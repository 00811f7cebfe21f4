// nameset.cpp -- sh_nameset_*: the names of a saved model as a hash set, matched against the name blob of a raw block (reader.cpp, the packed
// cache) without a Python string per line.  pyseer/enet_predict.py:160-174 looks every line's name up in the model's dict and pops it at
// its first hit; here a name is retired at its first hit, so a second line of the same name is not reported.  Host code only, one thread.
#include "../../include/seerhip.h"
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

namespace {
inline uint64_t load_tail(const unsigned char *p, size_t n) { uint64_t v = 0; memcpy(&v, p, n); return v; }
inline uint64_t hash_name(const char *s, size_t n)
{
    const unsigned char *p = reinterpret_cast<const unsigned char *>(s);
    uint64_t h = 0x9E3779B97F4A7C15ull ^ (uint64_t)n;
    for (; n >= 8; n -= 8, p += 8) { uint64_t v; memcpy(&v, p, 8); h = (h ^ v) * 0xFF51AFD7ED558CCDull; h ^= h >> 32; }
    if (n) { h = (h ^ load_tail(p, n)) * 0xFF51AFD7ED558CCDull; h ^= h >> 32; }
    h *= 0xC4CEB9FE1A85EC53ull; h ^= h >> 29;
    return h;
}
struct Slot { uint32_t hash; int32_t idx; };                         // the low half of the name's hash (the high bits choose the slot); idx < 0: empty
}

struct sh_nameset {
    std::vector<char> blob; std::vector<int64_t> off;                // the set's own copy of the names
    std::vector<Slot> table; uint64_t mask = 0;
    std::vector<uint8_t> met; int64_t left = 0;
};

extern "C" {
sh_nameset *sh_nameset_new(const char *blob, const int64_t *off, int64_t n)
{
    if (n < 0 || n > INT32_MAX || (n > 0 && (!blob || !off))) return nullptr;
    for (int64_t i = 0; i < n; ++i) if (off[i + 1] < off[i] || off[i] < 0) return nullptr;
    sh_nameset *s = new (std::nothrow) sh_nameset();
    if (!s) return nullptr;
    try {
        if (n) { s->blob.assign(blob + off[0], blob + off[n]); s->off.resize((size_t)n + 1); for (int64_t i = 0; i <= n; ++i) s->off[(size_t)i] = off[i] - off[0]; }
        else s->off.assign(1, 0);
        uint64_t cap = 16; while (cap < (uint64_t)n * 2 + 1) cap <<= 1;
        s->table.assign((size_t)cap, Slot{0, -1}); s->mask = cap - 1;
        s->met.assign((size_t)n, 0);
        for (int64_t i = 0; i < n; ++i) {
            const char *nm = s->blob.data() + s->off[(size_t)i]; const size_t len = (size_t)(s->off[(size_t)i + 1] - s->off[(size_t)i]);
            const uint64_t h = hash_name(nm, len);
            uint64_t at = (h >> 32) & s->mask; bool dup = false;
            while (s->table[(size_t)at].idx >= 0) {
                const Slot &t = s->table[(size_t)at];
                const size_t tl = (size_t)(s->off[(size_t)t.idx + 1] - s->off[(size_t)t.idx]);
                if (t.hash == (uint32_t)h && tl == len && memcmp(s->blob.data() + s->off[(size_t)t.idx], nm, len) == 0) { dup = true; break; }
                at = (at + 1) & s->mask;
            }
            if (dup) { s->met[(size_t)i] = 1; continue; }             // (a name given twice: its first entry stands, the second can never be met)
            s->table[(size_t)at] = Slot{(uint32_t)h, (int32_t)i};
            ++s->left;
        }
    } catch (const std::bad_alloc &) { delete s; return nullptr; }
    return s;
}

int64_t sh_nameset_match(sh_nameset *s, const char *blob, const int64_t *off, int64_t V, int64_t *row_idx, int32_t *model_idx)
{
    if (!s || V < 0 || (V > 0 && (!blob || !off || !row_idx || !model_idx))) return -1;
    int64_t hits = 0;
    // in groups of NS_GROUP names: hash them all and ask for their slots, then probe them in order.  A model of 10^5 names and more has a
    // table beyond the L2, and a probe that waits for memory costs several times the hash; the misses of a group overlap instead.
    enum { NS_GROUP = 32 };
    uint64_t hs[NS_GROUP];
    for (int64_t v0 = 0; v0 < V && s->left > 0; v0 += NS_GROUP) {
        const int g = (int)(V - v0 < NS_GROUP ? V - v0 : NS_GROUP);
        for (int k = 0; k < g; ++k) {
            if (off[v0 + k + 1] < off[v0 + k]) return -1;
            hs[k] = hash_name(blob + off[v0 + k], (size_t)(off[v0 + k + 1] - off[v0 + k]));
            __builtin_prefetch(&s->table[(size_t)((hs[k] >> 32) & s->mask)]);
        }
        for (int k = 0; k < g && s->left > 0; ++k) {
            const int64_t v = v0 + k;
            const char *nm = blob + off[v]; const size_t len = (size_t)(off[v + 1] - off[v]);
            const uint64_t h = hs[k];
            for (uint64_t at = (h >> 32) & s->mask; s->table[(size_t)at].idx >= 0; at = (at + 1) & s->mask) {
                const Slot &t = s->table[(size_t)at];
                if (t.hash != (uint32_t)h) continue;
                const size_t tl = (size_t)(s->off[(size_t)t.idx + 1] - s->off[(size_t)t.idx]);
                if (tl != len || memcmp(s->blob.data() + s->off[(size_t)t.idx], nm, len) != 0) continue;
                if (!s->met[(size_t)t.idx]) { s->met[(size_t)t.idx] = 1; --s->left; row_idx[hits] = v; model_idx[hits] = t.idx; ++hits; }
                break;
            }
        }
    }
    return hits;
}

int64_t sh_nameset_left(const sh_nameset *s) { return s ? s->left : -1; }
void sh_nameset_free(sh_nameset *s) { delete s; }
}
