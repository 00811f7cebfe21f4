"""A plain restatement of the hash and the table of the pattern de-duplication (csrc/dedup_kernels.hip: dd_mix, k_dd_hash, k_dd_insert,
k_dd_resolve), and the inputs that make it take its rare branches.  Test infrastructure.

A row is given as its 64-bit words, low word first (word i holds samples 64 i .. 64 i + 63, sample 64 i in bit 0), the last word masked to
the N sample bits: exactly what k_repack_bits leaves in T and k_dd_hash reads.

dd_mix is   h ^= w + C + (h << 6) + (h >> 2);  h *= M;  h ^= h >> 31   (mod 2^64).  The multiplication by the odd M and the xor-shift are
bijections of h, so two rows share a hash exactly when the value before the last multiplication is the same; for any prefix words, the last
word that reaches a chosen such value is  w = (P ^ h) - C - (h << 6) - (h >> 2).  colliding_rows solves that; rows_with_home_slot searches
random rows for given low bits of the hash."""
import numpy as np

SEED = 0x243F6A8885A308D3
GOLD = 0x9E3779B97F4A7C15
MULT = 0xBF58476D1CE4E5B9
DD_EMPTY = 0xFFFFFFFFFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF


def _premul(h, w):
    """the state after the xor of dd_mix, before its multiplication (Python ints)"""
    return h ^ ((w + GOLD + ((h << 6) & M64) + (h >> 2)) & M64)


def mix(h, w):
    """dd_mix on Python ints"""
    h = (_premul(h, w) * MULT) & M64
    return h ^ (h >> 31)


def hash_row(words):
    """k_dd_hash of one row (a sequence of ints): the table's empty marker maps to 0"""
    x = SEED
    for w in words:
        x = mix(x, int(w))
    return 0 if x == DD_EMPTY else x


def hash_rows(rows):
    """k_dd_hash of every row of a (V, n_words) uint64 array -> (V,) uint64"""
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    x = np.full(rows.shape[0], SEED, dtype=np.uint64)
    with np.errstate(over="ignore"):
        for i in range(rows.shape[1]):
            x = x ^ (rows[:, i] + np.uint64(GOLD) + (x << np.uint64(6)) + (x >> np.uint64(2)))
            x = x * np.uint64(MULT)
            x = x ^ (x >> np.uint64(31))
    x[x == np.uint64(DD_EMPTY)] = 0
    return x


def _random_words(rng, n, n_words):
    return rng.integers(0, 1 << 64, size=(n, n_words), dtype=np.uint64)


def colliding_rows(rng, n_words, k):
    """k distinct rows of n_words words with one hash: random prefix words, the last word solved for one common pre-multiplication value.
    -> (k, n_words) uint64.  The last word uses all of its 64 bits, so the sample count must be 64 * n_words."""
    assert n_words >= 2 and k >= 1
    target = int(rng.integers(0, 1 << 64, dtype=np.uint64))
    rows, seen = [], set()
    while len(rows) < k:
        prefix = tuple(int(w) for w in _random_words(rng, 1, n_words - 1)[0])
        if prefix in seen:
            continue
        h = SEED
        for w in prefix:
            h = mix(h, w)
        last = ((target ^ h) - GOLD - ((h << 6) & M64) - (h >> 2)) & M64
        assert _premul(h, last) == target
        seen.add(prefix)
        rows.append(prefix + (last,))
    return np.array(rows, dtype=np.uint64)


def rows_with_home_slot(rng, n_words, slots, wanted_slots, per_slot):
    """Random rows whose hash has the given low bits: for each slot s of wanted_slots, per_slot (an int, or one int per slot) distinct rows
    with hash & (slots - 1) == s, found by hashing random rows in bulk.  -> (rows (n, n_words) uint64, their home slots (n,) int64), grouped
    in the order of wanted_slots."""
    assert slots & (slots - 1) == 0
    wanted_slots = [int(s) for s in wanted_slots]
    need = [int(per_slot)] * len(wanted_slots) if np.isscalar(per_slot) else [int(n) for n in per_slot]
    found = [[] for _ in wanted_slots]
    while any(len(f) < n for f, n in zip(found, need)):
        cand = np.unique(_random_words(rng, 1 << 16, n_words), axis=0)
        home = (hash_rows(cand) & np.uint64(slots - 1)).astype(np.int64)
        for j, s in enumerate(wanted_slots):
            for r in cand[home == s]:
                if len(found[j]) < need[j] and not any(np.array_equal(r, o) for o in found[j]):
                    found[j].append(r)
    rows = np.array([r for f in found for r in f], dtype=np.uint64).reshape(-1, n_words)
    homes = np.array([s for f, s in zip(found, wanted_slots) for _ in f], dtype=np.int64)
    return rows, homes


def expected_representatives(rows):
    """The table's model.  The owner of a hash is the smallest row index that carries it (k_dd_insert: atomicMin); rep[v] = that owner if the
    two rows are equal, else v itself (k_dd_resolve: a different row under the owner's hash is tested on its own, and so is every duplicate
    of it).  -> (rep (V,) int64, the number of rows with rep[v] == v: what sh_dedup_info reports)."""
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    h = hash_rows(rows)
    _, first, inverse = np.unique(h, return_index=True, return_inverse=True)
    owner = first[inverse.reshape(-1)]
    same = (rows == rows[owner]).all(axis=1)
    rep = np.where(same, owner, np.arange(rows.shape[0]))
    return rep.astype(np.int64), int((rep == np.arange(rows.shape[0])).sum())


def table_slots(hashes, slots):
    """Linear probing as k_dd_insert does it, one key after the other: -> (the slot of each distinct hash, in order of first appearance; how
    many of them sit below their home slot, that is, were carried past the table's end).  Which key gets which slot depends on the order --
    on the device, on the scheduling -- but the set of occupied slots and the number of keys carried past the end do not."""
    assert slots & (slots - 1) == 0
    used, slot_of = set(), {}
    for h in (int(x) for x in np.asarray(hashes).reshape(-1)):
        if h in slot_of:
            continue
        s = h & (slots - 1)
        while s in used:
            s = (s + 1) & (slots - 1)
        used.add(s); slot_of[h] = s
    assert len(slot_of) < slots
    return slot_of, sum(1 for h, s in slot_of.items() if s < (h & (slots - 1)))


def words_of(K):
    """(V, N) 0/1 -> (V, ceil(N / 64)) uint64 words, the bits past N clear"""
    K = np.ascontiguousarray(K)
    V, N = K.shape
    b = np.zeros((V, (N + 63) // 64 * 8), dtype=np.uint8)
    p = np.packbits(K.astype(bool), axis=1, bitorder="little")
    b[:, :p.shape[1]] = p
    return b.view("<u8").astype(np.uint64)


def dense_of(rows, N):
    """the inverse: (V, n_words) uint64 -> (V, N) uint8"""
    b = np.ascontiguousarray(rows, dtype="<u8").view(np.uint8)
    return np.unpackbits(b, axis=1, bitorder="little")[:, :N]
