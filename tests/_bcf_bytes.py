"""Helper of the BCF tests and tools: VCF text -> the bytes of a BCF 2.2 file, written from the format's description alone (it shares no code
with pyseer_amd.input.BcfFile or csrc/vcf_reader.cpp: the three are checked against each other and against the text route).

All integers little-endian.  File: b"BCF\\2\\2", l_text u32, the header text NUL-terminated, then per record l_shared u32, l_indiv u32, the
shared block (CHROM i32, POS-1 i32, rlen i32, QUAL f32, n_allele<<16|n_info u32, n_fmt<<24|n_sample u32, ID, alleles, FILTER, INFO) and the
individual block (per FORMAT key: the key as a typed int, a descriptor with the per-sample count, n_sample x count values).  A typed value is
a descriptor byte (count<<4|type; count 15: a typed int with the count follows; types 0 void, 1 int8, 2 int16, 3 int32, 5 float, 7 char)
and its values.  GT values are (allele+1)<<1|phased; vectors shorter than the record's longest end in the end-of-vector mark."""
import struct

from _vcf_text import bgzf_bytes

_INT = {1: ("<b", -128, -127, -120, 127), 2: ("<h", -32768, -32767, -32760, 32767), 3: ("<i", -2147483648, -2147483647, -2147483640, 2147483647)}
_FLOAT_MISSING = struct.pack("<I", 0x7F800001)


def _int_type(values):
    for t in (1, 2, 3):
        if all(_INT[t][3] <= v <= _INT[t][4] for v in values if v is not None):
            return t
    raise ValueError("integer out of range")


def _desc(t, count):
    if count < 15:
        return bytes([count << 4 | t])
    return bytes([0xF0 | t]) + typed_ints([count])


def typed_ints(values, t=None):
    """A typed int vector; None is the type's missing value."""
    if not values:
        return b"\x00"
    t = t or _int_type(values)
    fmt, missing = _INT[t][0], _INT[t][1]
    return _desc(t, len(values)) + b"".join(struct.pack(fmt, missing if v is None else v) for v in values)


def typed_string(s):
    b = s.encode()
    return _desc(7, len(b)) + b


def _is_int(s):
    return s.lstrip("-").isdigit() and len(s) < 10


def _gt_values(field):
    """The values of one GT string: None for an empty field (no vector at all)."""
    if field == "":
        return None
    out, phased, tok = [], 0, ""
    for ch in field + "/":
        if ch in "/|":
            out.append(((int(tok) + 1) << 1 | phased) if tok.isdigit() else phased)
            phased, tok = (1 if ch == "|" else 0), ""
        else:
            tok += ch
    return out


def _format_block(key_index, values, n_sample, gt, gt_type):
    """One FORMAT field of the individual block.  values: the field's string per sample, None where the sample's field list ends before it."""
    if gt:
        memo = {}
        vecs = [None if v is None else memo[v] if v in memo else memo.setdefault(v, _gt_values(v)) for v in values]
        L = max([len(v) for v in vecs if v] + [1])
        t = gt_type
        fmt, missing, eov = _INT[t][0], _INT[t][1], _INT[t][2]
        body, packed = [], {}
        for i, (field, v) in enumerate(zip(values, vecs)):
            key = (field, i % 2 if v is None else 0)
            if key not in packed:
                if v is None:                             # an empty or absent field: by turns the missing value or nothing before the marks
                    v = [missing] if i % 2 else []
                packed[key] = b"".join(struct.pack(fmt, x) for x in v + [eov] * (L - len(v)))
            body.append(packed[key])
        return typed_ints([key_index]) + _desc(t, L) + b"".join(body)
    if all(v is None or v in (".", "") or _is_int(v) for v in values):
        ints = [int(v) if v not in (None, ".", "") else None for v in values]
        t = _int_type(ints)
        return typed_ints([key_index]) + _desc(t, 1) + b"".join(struct.pack(_INT[t][0], _INT[t][1] if v is None else v) for v in ints)
    raw = [(v or ".").encode() for v in values]
    L = max(len(b) for b in raw)
    return typed_ints([key_index]) + _desc(7, L) + b"".join(b.ljust(L, b"\0") for b in raw)


def _meta_id(line):
    body = line[line.index("<") + 1:]
    for part in body.rstrip(">").split(","):
        if part.startswith("ID="):
            return part[3:]
    return None


def bcf_from_vcf_text(text, idx=False, gt_int16=False, gt_last=False, minor=2, container=True, tweak=None):
    """BCF bytes (BGZF-wrapped unless container=False) of the VCF `text` (bytes or str).
    idx: every dictionary and contig line carries IDX=, and the indices are NOT the order of the lines (a reader that ignores IDX misreads).
    gt_int16: GT vectors as int16.  gt_last: GT is written after the record's other FORMAT fields.
    tweak(record_number, dict of the record's header words) may change chrom / n_sample before they are packed (malformed-record tests)."""
    if isinstance(text, bytes):
        text = text.decode()
    lines = [ln.rstrip("\r") for ln in text.split("\n")]
    meta = [ln for ln in lines if ln.startswith("##")]
    chrom_line = [ln for ln in lines if ln.startswith("#CHROM")][0]
    records = [ln.split("\t") for ln in lines if ln and not ln.startswith("#")]
    n_sample = max(0, len(chrom_line.split("\t")) - 9)
    # dictionary: PASS, then FILTER / INFO / FORMAT IDs in order of first appearance; undeclared ones get header lines, as bcftools adds them
    strings, contigs = ["PASS"], []
    for ln in meta:
        if ln.startswith(("##FILTER=<", "##INFO=<", "##FORMAT=<")) and _meta_id(ln) not in strings:
            strings.append(_meta_id(ln))
        elif ln.startswith("##contig=<") and _meta_id(ln) not in contigs:
            contigs.append(_meta_id(ln))
    for f in records:
        f += [""] * (9 - len(f))
        if f[0] not in contigs:
            contigs.append(f[0]); meta.append("##contig=<ID=%s>" % f[0])
        for x in f[6].split(";"):
            if x not in ("", ".") and x not in strings:
                strings.append(x); meta.append('##FILTER=<ID=%s,Description="added">' % x)
        for x in f[7].split(";"):
            k = x.split("=", 1)[0]
            if k not in ("", ".") and k not in strings:
                strings.append(k); meta.append('##INFO=<ID=%s,Number=.,Type=String,Description="added">' % k)
        for k in f[8].split(":"):
            if k not in ("", ".") and k not in strings:
                strings.append(k); meta.append('##FORMAT=<ID=%s,Number=.,Type=String,Description="added">' % k)
    if idx:                                               # PASS stays 0; the others count down from a number with a gap above the plain order
        s_index = {s: (0 if s == "PASS" else len(strings) + 3 - i) for i, s in enumerate(strings)}
        c_index = {c: len(contigs) + 1 - i for i, c in enumerate(contigs)}
        meta = [(ln[:-1] + ",IDX=%d>" % (c_index if ln.startswith("##contig") else s_index)[_meta_id(ln)])
                if ln.startswith(("##FILTER=<", "##INFO=<", "##FORMAT=<", "##contig=<")) else ln for ln in meta]
    else:
        s_index = {s: i for i, s in enumerate(strings)}
        c_index = {c: i for i, c in enumerate(contigs)}
    header = ("\n".join(meta + [chrom_line]) + "\n").encode() + b"\0"
    out = [b"BCF\x02" + bytes([minor]) + struct.pack("<I", len(header)) + header]
    for number, f in enumerate(records, 1):
        alleles = [f[3]] + ([] if f[4] in (".", "") else f[4].split(","))
        flt = [s_index[x] for x in f[6].split(";") if x not in ("", ".")]
        info = [x for x in f[7].split(";") if x not in ("", ".")]
        keys = [k for k in f[8].split(":") if k not in ("", ".")]
        fields = [(x.split(":") if x != "" else []) for x in (f[9:] + [""] * n_sample)[:n_sample]]
        order = list(range(len(keys)))
        if gt_last and "GT" in keys:
            order = [i for i in order if keys[i] != "GT"] + [keys.index("GT")]
        words = {"chrom": c_index[f[0]], "n_sample": n_sample}
        if tweak:
            tweak(number, words)
        shared = struct.pack("<iii", words["chrom"], int(f[1]) - 1, len(f[3]))
        shared += _FLOAT_MISSING if f[5] in (".", "") else struct.pack("<f", float(f[5]))
        shared += struct.pack("<II", len(alleles) << 16 | len(info), len(keys) << 24 | words["n_sample"])
        shared += typed_string("" if f[2] == "." else f[2]) + b"".join(typed_string(a) for a in alleles) + typed_ints(flt)
        for x in info:
            k, eq, v = x.partition("=")
            shared += typed_ints([s_index[k]]) + (b"\x00" if not eq else typed_ints([int(v)]) if _is_int(v) else typed_string(v))
        indiv = b""
        if n_sample:
            for i in order:
                vals = [(fl[i] if i < len(fl) else None) for fl in fields]
                indiv += _format_block(s_index[keys[i]], vals, n_sample, keys[i] == "GT", 2 if gt_int16 else 1)
        out.append(struct.pack("<II", len(shared), len(indiv)) + shared + indiv)
    data = b"".join(out)
    return bgzf_bytes(data) if container else data


WORKED_HEADER = ("##fileformat=VCFv4.2\n##contig=<ID=chr1>\n##contig=<ID=chr2>\n##FILTER=<ID=q10,Description=\"q\">\n"
                 "##INFO=<ID=AC,Number=1,Type=Integer,Description=\"a\">\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"g\">\n"
                 "##FORMAT=<ID=DP,Number=1,Type=Integer,Description=\"d\">\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tA\tB\tC\tD\n")
WORKED_LINE = "chr2\t101\t.\tAC\tT\t50\tq10\tAC=1\tDP:GT\t7:./.\t30:0|1\t29:0/0\t5:1\n"
WORKED_RECORD = bytes.fromhex("24000000 12000000 01000000 64000000 02000000 00004842 01000200 04000002"
                              "07 274143 1754 1101 1102 1101 1104 1107 1e1d05 1103 21 0000 0205 0202 0481".replace(" ", ""))
