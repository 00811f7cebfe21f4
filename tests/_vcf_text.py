"""Helpers of the VCF tests and tools: a BGZF writer (the container `bgzip` writes: gzip members of at most 64 KiB of text, each with a
'BC' extra field holding its compressed size, closed by the empty end-of-file member) and a seeded generator of VCF text."""
import struct
import zlib

_BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bgzf_bytes(data, block=0xff00, level=6):
    out = []
    for at in range(0, len(data), block):
        chunk = data[at:at + block]
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        body = c.compress(chunk) + c.flush()
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(body) + 25) + body
                   + struct.pack("<II", zlib.crc32(chunk) & 0xffffffff, len(chunk)))
    out.append(_BGZF_EOF)
    return b"".join(out)


def write_bgzf(path, data, level=6):
    with open(path, "wb") as f:
        f.write(bgzf_bytes(data, level=level))


def generated_vcf(n_pheno=5000, n_cols=5200, n_records=2000, seed=7, missing=0.03, contigs=("chr1", "chr2")):
    """(text bytes, phenotype sample names, column names).  Columns are a shuffle of the phenotyped samples and n_cols - n_pheno others; records
    mix 1-byte sample fields, 20-byte ones and a FORMAT with GT second, haploid and diploid calls, ~`missing` missing calls, and
    multi-allelic and filtered records."""
    import numpy as np
    rng = np.random.RandomState(seed)
    pheno = ["s%05d" % i for i in range(n_pheno)]
    cols = pheno + ["x%05d" % i for i in range(n_cols - n_pheno)]
    cols = [cols[i] for i in rng.permutation(n_cols)]
    rng.shuffle(pheno)
    lines = ["##fileformat=VCFv4.2", "##contig=<ID=chr1>", "##contig=<ID=chr2>",
             "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(cols)]
    pos = 0
    for r in range(n_records):
        contig = contigs[0] if r < (2 * n_records) // 3 else contigs[1]
        if r == (2 * n_records) // 3:
            pos = 0
        pos += int(rng.randint(1, 40))
        ref = "ACGT"[rng.randint(4)] * int(1 + (rng.randint(10) == 0) * rng.randint(1, 6))
        alt = "T" if ref[0] != "T" else "G"
        kind = rng.randint(20)
        if kind == 0:
            alt = alt + ",C" if ref[0] != "C" else alt + ",A"
        flt = ("PASS", ".", "q10", "q10;PASS", "LowQual;q10")[(0, 0, 0, 1, 2, 3, 4)[rng.randint(7)]] if rng.randint(4) == 0 else "PASS"
        af = rng.choice([0.001, 0.02, 0.1, 0.3, 0.6])
        carrier = rng.random_sample(n_cols) < af
        miss = rng.random_sample(n_cols) < missing
        style = r % 4
        if style == 0:                                   # 1-byte fields
            fmt = "GT"
            f = np.where(miss, ".", np.where(carrier, "1", "0"))
        elif style == 1:                                 # 20-byte fields, GT first
            fmt = "GT:AD:DP:GQ:PL"
            f = np.where(miss, ".:0,0:.:.:.0000000000", np.where(carrier, "1:0,186:186:99:1800,0", "0:186,0:186:99:0,1800"))
        elif style == 2:                                 # diploid, GT second
            fmt = "DP:GT:GQ"
            het = rng.random_sample(n_cols) < 0.5
            f = np.where(miss, np.where(het, "7:./.:3", "12:0/.:."), np.where(carrier, np.where(het, "30:0|1:99", "31:1/1:98"), "29:0/0:99"))
        else:                                            # mixed lengths, some empty fields, half-missing diploids
            fmt = "GT:DP"
            odd = rng.random_sample(n_cols) < 0.3
            f = np.where(miss, np.where(odd, "", "./0:1"), np.where(carrier, np.where(odd, "./1", "1:1234567"), np.where(odd, "0", "0/0:22")))
        if r % 97 == 5:
            fmt = "DP:GQ"                                # no GT at all
        lines.append("\t".join([contig, str(pos), ".", ref, alt, "50", flt, "AC=1", fmt]) + "\t" + "\t".join(f.tolist()))
    text = ("\n".join(lines) + "\n").encode()
    return text, pheno, cols
