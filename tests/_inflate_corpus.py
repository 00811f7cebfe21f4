"""The member corpus of the device-inflate tests (test_inflate_cpu.py, test_inflate_gpu.py): raw-DEFLATE members as BGZF carries them, well
formed and malformed, with zlib as the yardstick of both; the corpus file tools/inflate_core_check.cpp reads; BGZF files cut into members of
a chosen size, damaged and truncated.

Well-formed members: decoded sizes 0, 1, 2, 257, 258, 259, 32768, 32769, 65280, 65536 of
  one repeated byte (distance 1, length 258, overlapping copies), a period-3 pattern, a period-32768 pattern (the largest distance and
  the 13-extra-bit distance codes), random bytes, k-mer text, and an alphabet with counts 1, 1, 2, 4 .. 16384 coded without matches
  (Z_HUFFMAN_ONLY: its rare literals get 15-bit codes),
each at zlib levels 0 (stored blocks), 1, 6 and 9 (tiny inputs: fixed blocks); members of several blocks, made with Z_SYNC_FLUSH and
Z_FULL_FLUSH in mid-member (empty stored blocks, a stored block behind a block that did not end on a byte boundary); the empty member of
the 28-byte end marker.
Malformed members: one for every status of csrc/inflate_dev.h, written bit by bit or made by editing a well-formed one."""
import struct
import zlib

import numpy as np

SIZES = (0, 1, 2, 257, 258, 259, 32768, 32769, 65280, 65536)
LEVELS = (0, 1, 6, 9)
EOF_MEMBER = b"\x03\x00"                                  # the deflate body of BGZF's end marker


def yardstick(cdata, isize):
    """the bytes of a member by zlib; raises on anything that is not one whole raw-DEFLATE stream of isize bytes"""
    d = zlib.decompressobj(-15)
    out = d.decompress(cdata)
    if not d.eof:
        raise ValueError("the stream ends before its final block does")
    if len(out) != isize:
        raise ValueError("%d bytes, %d announced" % (len(out), isize))
    return out


def _deflate(data, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(data) + c.flush()


def _kmer_text():
    from _kmer_dev_corpus import corpus, sample_names
    text, _ = corpus(sample_names(65), n_lines=150, seed=3)
    return text


def _data(kind, n, rng, kmer):
    if kind == "byte":
        return b"A" * n
    if kind == "period3":
        return (b"abc" * (n // 3 + 1))[:n]
    if kind == "period32768":
        block = rng.randint(0, 256, size=32768).astype(np.uint8).tobytes()
        return (block * 3)[:n]
    if kind == "random":
        return rng.randint(0, 256, size=n).astype(np.uint8).tobytes()
    if kind == "kmer":
        return (kmer * (n // len(kmer) + 1))[:n]
    # "skewed": 16 byte values with counts 1, 1, 2, 4 .. 16384 -- 32 768 bytes whose Huffman code is 15 bits deep; coded without matches
    # (Z_HUFFMAN_ONLY) they fill zlib's block of 32 767 symbols, so the first block of the members of 32 768 bytes and more has 15-bit
    # literal codes (test_inflate_cpu.py checks it).  The most frequent value comes last: the symbol the block may lack costs no depth.
    pool = np.repeat(np.arange(16, dtype=np.uint8) + 65, [1] + [1 << i for i in range(15)])
    rng.shuffle(pool)
    last = int(np.nonzero(pool == 65 + 15)[0][-1])
    pool[last], pool[-1] = pool[-1], pool[last]
    return (pool.tobytes() * 2)[:n]


KINDS = ("byte", "period3", "period32768", "random", "kmer", "skewed")

# members of several blocks: name -> (level, where the text is cut, the flush after each piece)
FLUSHES = {"sync": (6, (5, 1000, 1001, 30000), (zlib.Z_SYNC_FLUSH,) * 4),
           "full": (9, (1, 2, 40000), (zlib.Z_FULL_FLUSH, zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH)),
           "twice": (1, (0, 0, 7, 7, 50000), (zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH, zlib.Z_SYNC_FLUSH, zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH)),
           "stored-sync": (0, (3, 70, 20000), (zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH, zlib.Z_SYNC_FLUSH))}
EMPTY_STORED = b"\x00\x00\xff\xff"                        # LEN, NLEN of the empty stored block a flush ends with, byte-aligned


def flush_member(name, kmer=None):
    """(deflate body, text, marks): marks = how many flushes put an empty stored block into the member, and so ended a block before it"""
    level, cuts, flushes = FLUSHES[name]
    kmer = kmer or _kmer_text()
    data = (kmer * (65536 // len(kmer) + 1))[:65536]
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    body, at, marks = b"", 0, 0
    for cut, fl in zip(cuts, flushes):
        piece = c.compress(data[at:cut]) + c.flush(fl)
        marks += piece.endswith(EMPTY_STORED)
        body += piece
        at = max(at, cut)
    return body + c.compress(data[at:]) + c.flush(), data, marks


def first_block_code_lengths(cdata):
    """(block type, the longest literal/length code, the longest distance code) of a member's first block; a dynamic block's header is
    walked as RFC 1951 3.2.7 lays it out (the code-length code, then HLIT + HDIST lengths with their repeat codes)"""
    bits = int.from_bytes(cdata[:400], "little")
    at = [0]

    def take(n):
        v = (bits >> at[0]) & ((1 << n) - 1)
        at[0] += n
        return v
    take(1)
    btype = take(2)
    if btype != 2:
        return btype, (9 if btype == 1 else 0), (5 if btype == 1 else 0)
    hlit, hdist, hclen = take(5) + 257, take(5) + 1, take(4) + 4
    cl = [0] * 19
    for s in _ORDER[:hclen]:
        cl[s] = take(3)
    # canonical codes of the code-length code: (length, code) -> symbol
    codes, code = {}, 0
    for ln in range(1, 8):
        for sym in range(19):
            if cl[sym] == ln:
                codes[(ln, code)] = sym
                code += 1
        code <<= 1
    lens = []
    while len(lens) < hlit + hdist:
        code = 0
        for ln in range(1, 8):
            code = (code << 1) | take(1)
            if (ln, code) in codes:
                break
        sym = codes[(ln, code)]
        if sym < 16:
            lens.append(sym)
        elif sym == 16:
            lens += [lens[-1]] * (3 + take(2))
        elif sym == 17:
            lens += [0] * (3 + take(3))
        else:
            lens += [0] * (11 + take(7))
    return btype, max(lens[:hlit]), max(lens[hlit:hlit + hdist])


def well_formed():
    """[(name, cdata, text)]"""
    rng = np.random.RandomState(20260)
    kmer = _kmer_text()
    out = []
    for kind in KINDS:
        for n in SIZES:
            data = _data(kind, n, rng, kmer)
            for level in LEVELS:
                strategy = zlib.Z_HUFFMAN_ONLY if kind == "skewed" else zlib.Z_DEFAULT_STRATEGY
                out.append(("%s-%d-l%d" % (kind, n, level), _deflate(data, level, strategy), data))
    # several blocks in one member
    for name in sorted(FLUSHES):
        body, data, _ = flush_member(name, kmer)
        out.append(("blocks-" + name, body, data))
    out.append(("eof-marker", EOF_MEMBER, b""))
    out.append(("one-code-set", _one_code_block().put(0, 1).bytes(), b""))
    # zlib's own matches stop 262 bytes short of the window, so the period-32768 members above hold no match at all: a period of 32 000 for
    # its 13-extra-bit distance codes, and the largest distance written by hand -- a stored block of 32 768 bytes, then a fixed block with
    # one match of length 258 (symbol 285) at distance 32 768 (symbol 29, extra bits all ones)
    block = rng.randint(0, 256, size=32768).astype(np.uint8).tobytes()
    far = (block[:32000] * 3)[:65536]
    out.append(("period32000-l6", _deflate(far, 6), far))
    b = _Bits().put(0, 1).put(0, 2).put(0, 5).put(32768, 16).put(32768 ^ 0xffff, 16)
    head = b.bytes() + block
    tail = _Bits().put(1, 1).put(1, 2).code(0xC0 + 5, 8).code(29, 5).put(8191, 13).code(0, 7).bytes()
    out.append(("distance-32768", head + tail, block + block[:258]))
    return out


class _Bits(object):
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value, nbits):                          # LSB first, as DEFLATE packs everything but Huffman codes
        self.acc |= (value & ((1 << nbits) - 1)) << self.n
        self.n += nbits
        return self

    def code(self, code, nbits):                          # a Huffman code: its first bit first
        for i in range(nbits - 1, -1, -1):
            self.put((code >> i) & 1, 1)
        return self

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def _dynamic_head(clens, hlit=257, hdist=1):
    """a final dynamic block's header with the code-length code `clens` (symbol -> length)"""
    hclen = max(4, 1 + max(_ORDER.index(s) for s in clens))
    b = _Bits().put(1, 1).put(2, 2).put(hlit - 257, 5).put(hdist - 1, 5).put(hclen - 4, 4)
    for s in _ORDER[:hclen]:
        b.put(clens.get(s, 0), 3)
    return b


# a complete code-length code over the symbols 0, 1, 2 and 18, two bits each: canonical codes 00, 01, 10, 11
_CL4 = {0: 2, 1: 2, 2: 2, 18: 2}
_CL4_CODE = {0: 0, 1: 1, 2: 2, 18: 3}


def _cl4(b, sym, extra=None):
    b.code(_CL4_CODE[sym], 2)
    if sym == 18:
        b.put(extra - 11, 7)
    return b


def _one_code_block():
    """a final dynamic block whose only code is end-of-block, one bit long (the incomplete set zlib accepts), and no distance code"""
    b = _dynamic_head(_CL4)
    _cl4(b, 18, 138); _cl4(b, 18, 118); _cl4(b, 1); _cl4(b, 0)
    return b


def malformed():
    """[(name, cdata, isize, status name in csrc/inflate_dev.h)]"""
    out = []
    out.append(("btype3", _Bits().put(1, 1).put(3, 2).bytes(), 0, "SHI_BTYPE"))
    stored = bytearray(_deflate(b"abc", 0))
    stored[3] ^= 0x01                                     # NLEN
    out.append(("stored-nlen", bytes(stored), 3, "SHI_STORED_LEN"))
    out.append(("codelen-oversubscribed", _dynamic_head({16: 1, 17: 1, 18: 1, 0: 1}).put(0, 16).bytes(), 0, "SHI_OVERSUBSCRIBED"))
    out.append(("codelen-incomplete", _dynamic_head({18: 2, 0: 2}).put(0, 16).bytes(), 0, "SHI_INCOMPLETE"))
    # literal/length lengths: symbol 0 and 256 two bits each and nothing else -- half the code space is unused
    b = _dynamic_head(_CL4)
    _cl4(b, 2); _cl4(b, 18, 138); _cl4(b, 18, 117); _cl4(b, 2); _cl4(b, 1)
    out.append(("litlen-incomplete", b.put(0, 16).bytes(), 0, "SHI_INCOMPLETE"))
    # symbols 0, 1 and 256 one bit each
    b = _dynamic_head(_CL4)
    _cl4(b, 1); _cl4(b, 1); _cl4(b, 18, 138); _cl4(b, 18, 116); _cl4(b, 1); _cl4(b, 1)
    out.append(("litlen-oversubscribed", b.put(0, 16).bytes(), 0, "SHI_OVERSUBSCRIBED"))
    out.append(("repeat-nothing", _dynamic_head({16: 1, 0: 1}).code(1, 1).put(0, 2).put(0, 16).bytes(), 0, "SHI_REPEAT"))
    b = _dynamic_head({18: 1, 0: 1})
    b.code(1, 1).put(127, 7).code(1, 1).put(127, 7)       # 138 + 138 zeros into 258 lengths
    out.append(("repeat-past-the-end", b.put(0, 16).bytes(), 0, "SHI_REPEAT"))
    # symbols 0 and 1 one bit each, no end-of-block code
    b = _dynamic_head(_CL4)
    _cl4(b, 1); _cl4(b, 1); _cl4(b, 18, 138); _cl4(b, 18, 117); _cl4(b, 1)
    out.append(("no-end-of-block", b.put(0, 16).bytes(), 0, "SHI_NO_EOB"))
    out.append(("hlit-287", _dynamic_head(_CL4, hlit=287).put(0, 16).bytes(), 0, "SHI_COUNTS"))
    out.append(("no-such-code", _one_code_block().put(0xffff, 16).bytes(), 0, "SHI_CODE"))
    fixed = lambda: _Bits().put(1, 1).put(1, 2)           # noqa: E731  (a final fixed block)
    lit_a = (0x30 + ord("a"), 8)
    out.append(("litlen-286", fixed().code(*lit_a).code(0xC0 + 6, 8).code(0, 7).bytes(), 1, "SHI_SYMBOL"))
    out.append(("litlen-287", fixed().code(*lit_a).code(0xC0 + 7, 8).code(0, 7).bytes(), 1, "SHI_SYMBOL"))
    out.append(("distance-30", fixed().code(*lit_a).code(1, 7).code(30, 5).code(0, 7).bytes(), 4, "SHI_SYMBOL"))
    out.append(("distance-31", fixed().code(*lit_a).code(1, 7).code(31, 5).code(0, 7).bytes(), 4, "SHI_SYMBOL"))
    out.append(("distance-before-start", fixed().code(*lit_a).code(1, 7).code(1, 5).code(0, 7).bytes(), 4, "SHI_DISTANCE"))
    rng = np.random.RandomState(7)
    kmer = _kmer_text()[:30000]
    good = _deflate(kmer, 6)
    out.append(("input-ends-in-a-symbol", good[:-1], len(kmer), "SHI_INPUT_END"))
    out.append(("clen-cut-short", good[:len(good) // 2], len(kmer), "SHI_INPUT_END"))
    out.append(("isize-understated", good, len(kmer) - 1, "SHI_OUTPUT_FULL"))
    out.append(("isize-overstated", good, len(kmer) + 1, "SHI_SHORT"))
    rnd = rng.randint(0, 256, size=300).astype(np.uint8).tobytes()
    out.append(("stored-understated", _deflate(rnd, 0), 299, "SHI_OUTPUT_FULL"))
    out.append(("stored-cut-short", _deflate(rnd, 0)[:200], 300, "SHI_INPUT_END"))
    out.append(("empty-input", b"", 0, "SHI_INPUT_END"))
    return out


def statuses():
    """name -> value of the ShInfStatus enumerators of csrc/inflate_dev.h"""
    import os
    import re
    h = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pyseer_amd", "csrc", "inflate_dev.h")).read()
    return {k: int(v) for k, v in re.findall(r"\b(SHI_[A-Z_]+) = (\d+)", h)}


def write_corpus_file(path):
    """the corpus for tools/inflate_core_check.cpp: "SHIC1\\n", a count, then per member kind (0 well formed, 1 malformed), clen, isize, the
    number of expected bytes, the compressed bytes and the expected ones (little-endian 32-bit fields)"""
    good, bad = well_formed(), malformed()
    with open(path, "wb") as f:
        f.write(b"SHIC1\n" + struct.pack("<I", len(good) + len(bad)))
        for _, c, text in good:
            f.write(struct.pack("<IIII", 0, len(c), len(text), len(text)) + c + text)
        for _, c, isize, _ in bad:
            f.write(struct.pack("<IIII", 1, len(c), isize, 0) + c)
    return len(good), len(bad)


# ---- the reader grid -----------------------------------------------------------------------------------------------------------------------
# lines of the corpus per member size: members of one byte are one member per byte of text
LINES = {1: 8, 100: 60, 40000: 150, 65280: 150}


def straddling_cases(n):
    """[(corpus arguments, member size)] under reader_slab=70000,reader_pad=32768: every member size for every n.  A BGZF slab is filled
    while 64 KB more would still fit, so with members of 1 or 100 bytes it holds 4.5 KB of text -- many small slabs, each carrying a tail
    longer than its own text.  The host route itself refuses a line longer than such a slab can ever complete, which of this corpus are
    only the two 40 000-byte lines: they go with the large members at n = 300, and the small members get the corpus without them."""
    big = dict(n_lines=60 if n <= 9 else 300, seed=5, long_tokens=2 if n == 300 else 0)
    return [(dict(n_lines=LINES[1], seed=5), 1), (dict(n_lines=LINES[100], seed=5), 100), (big, 40000), (big, 65280)]


# ---- BGZF files -----------------------------------------------------------------------------------------------------------------------------
def members_of(data):
    """[(offset, total size, isize)] of a BGZF file's members"""
    out, at = [], 0
    while at < len(data):
        bs = struct.unpack_from("<H", data, at + 16)[0] + 1
        out.append((at, bs, struct.unpack_from("<I", data, at + bs - 4)[0]))
        at += bs
    return out


def flip_member_byte(data, which):
    """the file with one byte of member `which`'s deflate body changed"""
    at, bs, _ = members_of(data)[which]
    bad = bytearray(data)
    bad[at + 18 + (bs - 26) // 2] ^= 0x10
    return bytes(bad)


def truncate_last_member(data):
    """the file without its end marker and without the last 9 bytes of its last member"""
    at, bs, _ = members_of(data)[-2]
    return data[:at + bs - 9]
