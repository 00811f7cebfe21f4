"""The k-mer corpus of the device-route tests (test_kmer_dev_cpu.py, test_kmer_dev_gpu.py): lines made to meet every clause of the tokenising
rule, the four containers, and the comparison of two readers block by block."""
import gzip

import numpy as np

from _vcf_text import bgzf_bytes

# names in the order a small sample count takes them: 1, 8, 9, 16, 17 and 40 bytes; #3 and #4 differ only in length (and agree in their first
# 16 bytes), #5 and #6 have the same length and agree in their first 16 bytes; #8 repeats #1 (the first occurrence wins: bit 8 is never set)
SPECIAL = ["a", "sample_8", "sample__9", "sample_sixteen_x", "sample_sixteen_xy", "sixteen_bytes_ab_01", "sixteen_bytes_ab_02",
           "a_name_of_forty_bytes_for_the_long_path_", "sample_8"]
OTHERS = ["nophenotype", "x", "sample_", "sample_sixteen_xyz", "sixteen_bytes_ab_0", "A", "sample_8_"]      # in the file, without a phenotype


def sample_names(n, seed=0):
    """n phenotype names: the special ones as far as n reaches, then plain ones; shuffled"""
    names = (SPECIAL + ["s%05d" % i for i in range(max(0, n - len(SPECIAL)))])[:n]
    rng = np.random.RandomState(seed + n)
    return [names[i] for i in rng.permutation(n)]


def corpus(names, n_lines=400, seed=0, long_tokens=0):
    """text bytes of at most 2000 lines over `names` (see the module docstring of test_kmer_dev_gpu.py for what they hold).
    long_tokens: that many extra lines with 40 000 bytes of sample tokens each."""
    rng = np.random.RandomState(seed)
    uniq = sorted(set(names))
    n = len(uniq)

    def kmer():
        return "".join("ACGT"[i] for i in rng.randint(0, 4, size=rng.randint(9, 41)))

    def tok(s):
        r = rng.randint(0, 20)
        if r == 0:
            return s                                        # no ':'
        if r == 1:
            return s + ":3:4:5"                             # several
        if r == 2:
            return s + ":"
        return "%s:%d" % (s, rng.randint(1, 500))

    def sep():
        r = rng.randint(0, 12)
        return " " if r > 2 else ("\t", "   ", " \t ")[r]

    def tokens(carriers, extras=3):
        t = [tok(uniq[i]) for i in carriers]
        t += [tok(OTHERS[i]) for i in rng.randint(0, len(OTHERS), size=extras)]
        if len(carriers):
            t += [tok(uniq[carriers[0]])] * 2               # a sample repeated within a line
        t.append(":3")                                      # a token that is only a count
        order = rng.permutation(len(t))
        out = ""
        for j in order:
            out += sep() + t[j]
        return out

    lines = []
    for i in range(n_lines):
        k = (0, n, 1, n - 1)[i] if i < 4 else rng.randint(0, n + 1)
        carriers = rng.permutation(n)[:max(0, min(n, k))]
        eol = "\r" if i % 7 == 3 else ""
        lines.append(kmer() + " |" + tokens(carriers) + ("" if i % 5 else " ") + eol)
    some = rng.permutation(n)[:max(1, n // 2)]
    rest = [i for i in range(n) if i not in set(some.tolist())]
    lines[10:10] = [
        kmer(),                                                                  # no '|'
        kmer() + " " + " ".join(tok(s) for s in uniq[:5]),                       # no '|', tokens all the same
        kmer() + " |",                                                           # empty segments
        kmer() + " | ",
        kmer() + " ||" + tokens(some),
        kmer() + "|" + uniq[0] + ":1",                                           # nothing around the bar
        kmer() + " |" + tokens(some) + " | " + " ".join(tok(uniq[i]) for i in rest) + " | " + uniq[0] + ":2",   # what follows a second '|' does not count
        kmer() + " |" + tokens(some) + "|" + uniq[-1],
        "",                                                                      # a blank line
        kmer() + "\t|\t" + "\t".join(tok(s) for s in uniq) + "\r",               # tabs, everybody, CRLF
        kmer() + " | " + (" " * 300) + uniq[0] + ":1" + ("\t" * 200),            # runs of blanks
    ]
    for j in range(long_tokens):
        body = ""
        while len(body) < 40000:
            body += sep() + tok(uniq[rng.randint(0, n)] if rng.randint(0, 4) else OTHERS[rng.randint(0, len(OTHERS))])
        # the first one begins 32 000 bytes or a little more into the text: with slabs of 70 000 bytes and a pad of 32 768 more than the pad of
        # it lies in the first slab, so it is copied out (the reader's `bridge`); the second falls where it falls
        at, size = len(lines) * 2 // 3, 0
        if j == 0:
            for at, ln in enumerate(lines):
                size += len(ln) + 1
                if size >= 32000:
                    at += 1
                    break
        lines.insert(at, kmer() + " |" + body)
    assert len(lines) <= 2000
    last = kmer() + " | " + uniq[0] + ":7 " + uniq[-1]                            # the last line has no newline
    return ("\n".join(lines) + "\n" + last).encode(), len(lines) + 1


def containers(text):
    """name -> file bytes: plain text, one gzip member, three concatenated members, BGZF"""
    cut1, cut2 = len(text) // 3, 2 * len(text) // 3 + 5
    return {"plain": text, "gzip": gzip.compress(text, 6),
            "gzip3": gzip.compress(text[:cut1], 6) + gzip.compress(text[cut1:cut2], 1) + gzip.compress(text[cut2:], 9),
            "bgzf": bgzf_bytes(text, block=40000)}


def read_blocks(path, names, block_size, engine=None, max_name=256):
    """([(bits, counts, blob, off)], dev_stats or None) of one pass; engine as NativeKmerReader takes it"""
    from pyseer_amd.input import NativeKmerReader
    r = NativeKmerReader(path, names, block_size, max_name, engine=engine)
    try:
        blocks = [(b.copy(), c.copy(), blob, off) for b, c, blob, off in r.raw_blocks()]
        stats = r.dev_stats() if engine is not None else None
    finally:
        r.close()
    return blocks, stats


def assert_same_blocks(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert g[2] == w[2], (what, i, "names")
        assert np.array_equal(g[3], w[3]), (what, i, "offsets")
        assert np.array_equal(g[1], w[1]), (what, i, "counts", np.nonzero(g[1] != w[1])[0][:5])
        assert np.array_equal(g[0], w[0]), (what, i, "bits")
