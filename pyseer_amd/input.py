"""Variant stream and loaders, mirroring pyseer/input.py's contracts for k-mer and Rtab input.

The generators keep the reference's tuple layouts (iter_variants: the 16-tuple that is the argument list of
fixed_effects_regression, input.py:608-620; load_var_block: (variants, variant_mat, eof), input.py:678-707) so existing
callers keep working; `iter_packed_blocks` is the feed of the GPU driver: the same parsing, but presence goes straight
into packed bit rows.  VCF input (pyseer/input.py:250-266, 383-407, 455-503) is read as text -- plain, gzip or BGZF -- by `VcfFile`
(the `--python-reader` path and the yardstick) or by the native reader whose sample columns are tokenised on the device (`NativeVcfReader`,
csrc/vcf_reader.cpp + csrc/vcf_kernels.hip).  BCF 2.1 / 2.2, sniffed from the decoded bytes, takes the same two routes: `BcfFile`, and the
native reader, which sends each record's GT vector to k_bcf_gt_pack.  No tabix index is read: burden regions are assigned in one pass over the file.
The CallBlocks of the native VCF / BCF / Rtab readers can be kept in a call cache (`CallCacheWriter`, `open_call_cache`, `iter_call_cache_blocks`:
--save-calls / --load-calls) and served to any subset or order of its samples, as the packed cache serves k-mer rows.
"""
import binascii
import gzip
import hashlib
import os
import re
import struct
import sys

import numpy as np
import pandas as pd

from . import classes as var_obj
from . import _route
from .packing import row_bytes_for


# ---------------------------------------------------------------------------------------------------------------
# loaders (once per run)
# ---------------------------------------------------------------------------------------------------------------
def _read_indexed_table(path, what, **kw):
    t = pd.read_csv(path, index_col=0, sep='\t', **kw)
    t.index = t.index.astype(str)
    if np.any(t.index.duplicated()):
        sys.stderr.write('%s file contains duplicated sample names\n' % what)
        sys.exit(1)
    return t


def load_phenotypes(infile, column):
    """pandas.Series of phenotypes indexed by sample (input.py:24-59): last column unless `column` is named."""
    p = pd.read_csv(infile, index_col=0, sep='\t')
    if p.shape[1] < 1:
        sys.stderr.write('Phenotype file must contain at least one phenotype column\n')
        sys.exit(1)
    p.index = p.index.astype(str)
    if np.any(p.index.duplicated()):
        sys.stderr.write('Phenotype file contains duplicated sample names\n')
        sys.exit(1)
    p = (p[p.columns[-1]] if column is None else p[column]).dropna()
    if not pd.api.types.is_numeric_dtype(p.values.dtype):
        sys.stderr.write('Phenotypes must be numeric\n')
        sys.exit(1)
    return p


def cmdscale(D):
    """Classical MDS (cmdscale.py:15-54): double-centre the squared distances, keep positive-eigenvalue axes."""
    D = np.asarray(D, dtype=float)
    n = D.shape[0]
    H = np.eye(n) - np.ones((n, n)) / n
    B = -H.dot(D ** 2).dot(H) / 2
    evals, evecs = np.linalg.eigh(B)
    order = np.argsort(evals)[::-1]
    evals, evecs = evals[order], evecs[:, order]
    pos = evals > 0
    return evecs[:, pos] * np.sqrt(evals[pos]), evals[pos]


def load_structure(infile, p, max_dimensions, mds_type="classic", n_cpus=1, seed=None):
    """Distance matrix -> MDS projection restricted to phenotyped samples, columns scaled by max-abs (input.py:62-137)."""
    m = _read_indexed_table(infile, 'Structure')
    sys.stderr.write("Structure matrix has dimension " + str(m.shape) + "\n")
    keep = p.index.intersection(m.index).intersection(m.columns)
    m = m.loc[keep, keep]
    if len(keep) == 0:
        sys.stderr.write('None of the phenotyped samples were found in population structure matrix\n')
        sys.exit(1)
    if mds_type == "classic":
        projection, _ = cmdscale(m.values)
    else:
        from sklearn import manifold
        metric = mds_type != "non-metric"
        if mds_type not in ("metric", "non-metric"):
            sys.stderr.write("Unsupported mds type chosen. Assuming metric\n")
        mds = manifold.MDS(n_components=max_dimensions, metric=metric, n_jobs=n_cpus, random_state=seed,
                           dissimilarity='precomputed')
        projection = mds.fit_transform(m.values)
    m = pd.DataFrame(projection, index=m.index)
    for i in range(m.shape[1]):
        m[i] = m[i] / max(abs(m[i]))
    return m


def load_covariates(infile, covariates, p):
    """Covariate table -> design columns: 'Nq' quantitative, 'N' categorical dummy-encoded (input.py:184-248)."""
    c = _read_indexed_table(infile, 'Covariate', header=0)
    if len(p.index.difference(c.index)) > 0:
        sys.stderr.write("All samples with a phenotype must be present in covariate file\n")
        sys.exit(1)
    c = c.loc[p.index.intersection(c.index)]
    if covariates is None:
        return pd.DataFrame([])
    cols = []
    for col in covariates:
        cnum = int(col.rstrip('q'))
        if cnum == 1 or cnum > c.shape[1] + 1:
            sys.stderr.write('Covariates columns values should be > 1 and less than or equal to total number of ' +
                             'columns (%d)\n' % (c.shape[1] + 1))
            return None
        series = c.iloc[:, cnum - 2]
        if col[-1] == 'q':
            cols.append(series)
        else:
            categories = set(series)
            categories.pop()                       # one level is the reference class (arbitrary, as in the reference)
            for i, categ in enumerate(categories):
                cols.append(pd.Series([1 if x == categ else 0 for x in series.values], index=c.index,
                                      name=c.columns[cnum - 2] + "_" + str(i)))
    return pd.concat(cols, axis=1) if cols else pd.DataFrame([])


def load_lineage(infile, p):
    """Cluster file (sample<ws>cluster) -> (n x clusters 0/1 matrix, sorted labels) (input.py:140-181)."""
    names, labels = [], []
    for line in open(infile):
        f = line.rstrip().split()
        names.append(f[0]); labels.append(f[1])
    lin = pd.Series(labels, index=pd.Index(names).astype(str))
    lin = lin.loc[~lin.index.duplicated()]
    if len(p.index.difference(lin.index)) > 0:
        sys.stderr.write("All samples with a phenotype must be present in lineage file\n")
        sys.exit(1)
    lin = lin.loc[p.index.intersection(lin.index)]
    lineages = sorted(set(lin.values))
    mat = np.stack([(lin.values == c).astype(int) for c in lineages], axis=1)
    return mat, lineages


def load_burden(infile, burden_regions):
    """Append (name, [region, ...]) per line `NAME region[,region...]` of the regions file to burden_regions (input.py:250-266)."""
    with open(infile, "r") as region_file:
        for line in region_file:
            name, regions = line.rstrip().split()
            burden_regions.append((name, regions.split(',')))


# ---------------------------------------------------------------------------------------------------------------
# VCF as text ("VCF input"): what the reference takes from pysam's records is the contig, the position, the alleles, FILTER and
# every sample's GT (input.py:455-503); all of it is in the tab-separated line.
# ---------------------------------------------------------------------------------------------------------------
VCF_KEPT, VCF_MULTI, VCF_FILTERED = 0, 1, 2          # skip reasons (include/seerhip.h sh_vcf_next)
GT_ABSENT, GT_PRESENT, GT_MISSING = 0, 1, 2


def gt_code(gt):
    """The three-way code of one GT string: present as soon as one haplotype is a non-zero allele index (any digit 1-9: separators are
    `/` and `|`, everything else in a well-formed GT is digits and `.`); otherwise absent if the LAST haplotype holds a 0, else missing."""
    for c in gt:
        if '1' <= c <= '9':
            return GT_PRESENT
    last = gt[max(gt.rfind('/'), gt.rfind('|')) + 1:]
    return GT_ABSENT if '0' in last else GT_MISSING


class VcfRecord(object):
    __slots__ = ("contig", "pos", "ref", "alt", "skip", "name", "gt_index", "fields")

    def __init__(self, line):
        f = line.rstrip('\r\n').split('\t')
        f += [''] * (9 - len(f))
        self.contig, self.pos, self.ref, self.alt = f[0], int(f[1]), f[3], f[4]
        flt = [x for x in f[6].split(';') if x not in ('', '.')]
        self.skip = VCF_MULTI if ',' in self.alt else (VCF_FILTERED if (flt and 'PASS' not in flt) else VCF_KEPT)
        self.name = "_".join([self.contig, f[1], self.ref] + ([] if self.alt in ('.', '') else [self.alt]))
        fmt = f[8].split(':')
        self.gt_index = fmt.index('GT') if 'GT' in fmt else -1
        self.fields = f[9:]

    def name_all_alleles(self):
        """contig_pos_ref_alt1_alt2...: the name pysam's alleles give a record with several ALTs (read_vcf_var, pyseer/input.py:470-471)."""
        return self.name.replace(',', '_') if self.skip == VCF_MULTI else self.name

    def codes(self, n_cols, cache):
        """GT_* code of every sample column (a record with fewer fields than the header has columns: the rest are empty = missing)."""
        gi = self.gt_index
        if gi < 0:
            return [GT_MISSING] * n_cols
        out = []
        for field in self.fields[:n_cols]:
            c = cache.get(field) if gi == 0 else None
            if c is None:
                sub = field.split(':', gi + 1)
                c = gt_code(sub[gi]) if gi < len(sub) else GT_MISSING
                if gi == 0 and len(cache) < 65536:
                    cache[field] = c
            out.append(c)
        out += [GT_MISSING] * (n_cols - len(out))
        return out


def _open_text(path):
    """Text handle of a plain, gzip or BGZF file, sniffed from the magic bytes (BGZF is a series of gzip members: gzip reads it)."""
    with open(path, "rb") as fh:
        magic = fh.read(2)
    return gzip.open(path, "rt") if magic == b"\x1f\x8b" else open(path, "r")


class VcfFile(object):
    """Iterator over the records of a VCF text file, with the region query burden testing needs.  `samples`: the header's columns."""

    def __init__(self, path):
        self.path = path
        self._fh = _open_text(path)
        self.samples = None
        for line in self._fh:
            if line.startswith('#CHROM'):
                self.samples = [str(x) for x in line.rstrip('\r\n').split('\t')[9:]]
                break
            if not line.startswith('#'):
                break
        if self.samples is None:
            raise ValueError('%s has no #CHROM header line; is this a VCF file?' % path)
        self._cache = {}
        self._indexed = {}                # (contig, start, end) -> records whose span meets [start, end), in file order

    def __iter__(self):
        return self

    def __next__(self):
        for line in self._fh:
            if line.rstrip('\r\n') and not line.startswith('#'):
                return VcfRecord(line)
        raise StopIteration

    def close(self):
        self._fh.close()

    def apply(self, rec, d):
        """read_vcf_var (input.py:455-503) on the dictionary d shared by the records of a burden region: present stays; otherwise the last
        applied record decides between missing and absent.  Returns the record's name, None if it is skipped."""
        if rec.skip == VCF_MULTI:
            sys.stderr.write("Multiple alleles at %s_%d. Skipping\n" % (rec.contig, rec.pos))
            return None
        if rec.skip:
            return None
        for sample, c in zip(self.samples, rec.codes(len(self.samples), self._cache)):
            if c == GT_PRESENT:
                d[sample] = 1
            elif c == GT_MISSING:
                if sample not in d:
                    d[sample] = np.nan
            elif sample in d and d[sample] != 1:
                del d[sample]
        return rec.name

    def prepare(self, intervals):
        """One pass over the file for all the (contig, start, end) not looked up before: no index file is read."""
        import bisect
        todo = [iv for iv in dict.fromkeys(intervals) if iv not in self._indexed]
        if not todo:
            return
        by_contig = {}
        for iv in todo:
            self._indexed[iv] = []
            by_contig.setdefault(iv[0], []).append(iv)
        starts, longest = {}, {}
        for c, ivs in by_contig.items():
            ivs.sort(key=lambda iv: iv[1])
            starts[c] = [iv[1] for iv in ivs]
            longest[c] = max(iv[2] - iv[1] for iv in ivs)
        with _open_text(self.path) as fh:
            for line in fh:
                if line.startswith('#') or not line.rstrip('\r\n'):
                    continue
                tab = line.index('\t')
                contig = line[:tab]
                if contig not in by_contig:
                    continue
                f = line.split('\t', 5)
                a = int(f[1]) - 1
                b = a + len(f[3])
                ivs = by_contig[contig]
                rec = None
                for j in range(bisect.bisect_left(starts[contig], a - longest[contig]), bisect.bisect_left(starts[contig], b)):
                    if ivs[j][1] < b and a < ivs[j][2]:
                        rec = rec or VcfRecord(line)
                        self._indexed[ivs[j]].append(rec)

    def fetch(self, contig, start, end):
        """The records whose span [POS-1, POS-1+len(REF)) meets [start, end), in file order (what pysam's fetch returns from the index)."""
        self.prepare([(contig, start, end)])
        return self._indexed[(contig, start, end)]


# ---------------------------------------------------------------------------------------------------------------
# BCF 2.1 / 2.2 ("BCF input"): the binary form of the same records.  `BcfFile` is the `--python-reader` path and the yardstick of
# the native BCF route (csrc/vcf_reader.cpp "BCF" + k_bcf_gt_pack); it parses with `struct` and shares nothing with the C++.
# ---------------------------------------------------------------------------------------------------------------
_BCF_WIDTH = {1: 1, 2: 2, 3: 4, 5: 4, 7: 1}
_BCF_INT = {1: ('<i1', 0x80, 0x81), 2: ('<i2', 0x8000, 0x8001), 3: ('<i4', 0x80000000, 0x80000001)}   # dtype, missing, end of vector


def _open_binary(path):
    with open(path, "rb") as fh:
        magic = fh.read(2)
    return gzip.open(path, "rb") if magic == b"\x1f\x8b" else open(path, "rb")


def is_bcf(path):
    """True if the decoded bytes of `path` (plain, gzip or BGZF) start with the BCF magic: the name of the file does not count."""
    try:
        with _open_binary(path) as fh:
            return fh.read(3) == b"BCF"
    except (OSError, EOFError):
        return False


def _bcf_meta(line):
    """(ID, IDX or None) of a `##KIND=<key=value,...>` header line; values may be quoted."""
    body = line[line.index('<') + 1:]
    out, i, n = {}, 0, len(body)
    while i < n and body[i] != '>':
        j = i
        while j < n and body[j] not in '=,>':
            j += 1
        key, val = body[i:j], ''
        if j < n and body[j] == '=':
            j += 1
            if j < n and body[j] == '"':
                j += 1
                while j < n and body[j] != '"':
                    if body[j] == '\\' and j + 1 < n:
                        j += 1
                    val += body[j]
                    j += 1
                j += 1
            else:
                k = j
                while j < n and body[j] not in ',>':
                    j += 1
                val = body[k:j]
        out[key] = val
        i = j + 1 if j < n and body[j] == ',' else j
    idx = out.get('IDX')
    return out.get('ID'), (int(idx) if idx is not None and idx.isdigit() and len(idx) < 10 else None)


class _BcfCursor(object):
    """Typed values out of one block of a record; every read is bounded by the block."""

    def __init__(self, buf, what, number):
        self.b, self.at, self.what, self.number = buf, 0, what, number

    def fail(self, thing):
        raise ValueError("BCF: record %d: %s runs past the %s block" % (self.number, thing, self.what))

    def take(self, n, thing):
        if n < 0 or self.at + n > len(self.b):
            self.fail(thing)
        self.at += n
        return self.b[self.at - n:self.at]

    def scalar(self, thing):
        d = self.take(1, thing)[0]
        if d >> 4 != 1 or d & 15 not in (1, 2, 3):
            self.fail(thing)
        w = _BCF_WIDTH[d & 15]
        return int.from_bytes(self.take(w, thing), "little", signed=True)

    def descriptor(self, thing):
        d = self.take(1, thing)[0]
        count = d >> 4
        if count == 15:
            count = self.scalar(thing)
            if count < 0:
                self.fail(thing)
        return d & 15, count

    def string(self, thing):
        t, count = self.descriptor(thing)
        if t == 0:
            return ''
        if t != 7:
            self.fail(thing)
        return self.take(count, thing).decode()


class BcfRecord(object):
    """One BCF record with VcfRecord's interface: contig, pos (1-based), ref, alt (the ALTs joined by commas), skip, name, codes()."""
    __slots__ = ("contig", "pos", "ref", "alt", "skip", "name", "number", "n_sample", "n_fmt", "indiv", "gt_key")

    def __init__(self, number, shared, indiv, contigs, gt_key, n_cols):
        if len(shared) < 24:
            raise ValueError("BCF: record %d: a shared block shorter than its fixed part" % number)
        chrom, pos0, _rlen, _qual, ai, fs = struct.unpack_from("<iiifII", shared, 0)
        n_allele, self.n_fmt, self.n_sample = ai >> 16, fs >> 24, fs & 0xffffff
        if chrom not in contigs:
            raise ValueError("BCF: record %d: CHROM index %d names no ##contig line of the header" % (number, chrom))
        if self.n_sample not in (0, n_cols):
            raise ValueError("BCF: record %d: n_sample is %d, the header has %d sample columns" % (number, self.n_sample, n_cols))
        c = _BcfCursor(shared[24:], "shared", number)
        c.string("ID")
        alleles = [c.string("an allele") for _ in range(n_allele)]
        t, count = c.descriptor("FILTER")
        flt = []
        if t != 0:
            if t not in _BCF_INT:
                c.fail("FILTER")
            dt, mis, eov = _BCF_INT[t]
            v = np.frombuffer(c.take(count * _BCF_WIDTH[t], "FILTER"), dtype=dt.replace('i', 'u'))
            flt = [int(x) for x in v if x != mis and x != eov]
        self.number, self.indiv, self.gt_key = number, indiv, gt_key
        self.contig, self.pos = contigs[chrom], pos0 + 1
        self.ref, self.alt = (alleles[0] if alleles else ''), ",".join(alleles[1:])
        self.skip = VCF_MULTI if n_allele > 2 else (VCF_FILTERED if (flt and 0 not in flt) else VCF_KEPT)
        self.name = "_".join([self.contig, str(self.pos), self.ref] + ([self.alt] if n_allele > 1 else []))

    def name_all_alleles(self):
        return self.name.replace(',', '_') if self.skip == VCF_MULTI else self.name

    def _gt(self):
        """The GT vector as an (n_sample, L) array of unsigned values with its missing and end-of-vector marks, or None."""
        if self.n_sample == 0:
            return None
        c = _BcfCursor(self.indiv, "individual", self.number)
        for _ in range(self.n_fmt):
            key = c.scalar("a FORMAT field")
            t, count = c.descriptor("a FORMAT field")
            if t != 0 and t not in _BCF_WIDTH:
                raise ValueError("BCF: record %d: a FORMAT field of unknown type %d" % (self.number, t))
            data = c.take(count * _BCF_WIDTH.get(t, 0) * self.n_sample, "a FORMAT field")
            if key == self.gt_key and self.gt_key is not None:
                if t == 0 or count == 0:
                    return None
                if t not in _BCF_INT:
                    raise ValueError("BCF: record %d: GT is not a vector of integers" % self.number)
                dt, mis, eov = _BCF_INT[t]
                return np.frombuffer(data, dtype=dt.replace('i', 'u')).reshape(self.n_sample, count).astype(np.int64), mis, eov
        return None

    def codes(self, n_cols, cache):
        g = self._gt()
        if g is None:
            return [GT_MISSING] * n_cols
        v, mis, eov = g
        live = np.logical_and.accumulate(v != eov, axis=1)          # the values before the end-of-vector mark
        allele = (v >> 1) - 1
        present = (live & (v != mis) & (allele >= 1)).any(axis=1)
        n_live = live.sum(axis=1)
        last = v[np.arange(v.shape[0]), np.maximum(n_live - 1, 0)]
        absent = ~present & (n_live > 0) & (last != mis) & ((last >> 1) == 1)
        return np.where(present, GT_PRESENT, np.where(absent, GT_ABSENT, GT_MISSING)).tolist()


class BcfFile(VcfFile):
    """VcfFile's interface over a BCF 2.1 / 2.2 file (plain, gzip or BGZF bytes): samples, iteration, apply, prepare, fetch."""

    def __init__(self, path):
        self.path = path
        self._cache = {}
        self._indexed = {}
        self._fh, self._contigs, self._gt_key, self.samples = self._open(path)
        self._number = 0

    @staticmethod
    def _open(path):
        fh = _open_binary(path)
        head = fh.read(9)
        if len(head) < 9 or head[:3] != b"BCF":
            raise ValueError('%s: not a BCF file, or one that ends inside its head' % path)
        if head[3] == 4:
            raise ValueError('%s is BCF1 (BCF\\4), which is not read: BCF 2.1 and 2.2 are' % path)
        if head[3] != 2:
            raise ValueError('%s: BCF major version %d is not read: BCF 2.1 and 2.2 are' % (path, head[3]))
        if head[4] not in (1, 2):
            raise ValueError('%s: BCF minor version %d is not read: BCF 2.1 and 2.2 are' % (path, head[4]))
        l_text = struct.unpack("<I", head[5:9])[0]
        text = fh.read(l_text)
        if len(text) < l_text:
            raise ValueError('%s: BCF: the file ends inside its header text' % path)
        text = text.split(b"\0", 1)[0].decode()
        strings, contigs, samples, n_contig = {"PASS": 0}, {}, None, 0
        for line in text.split("\n"):
            line = line.rstrip("\r")
            if line.startswith("##contig=<"):
                name, idx = _bcf_meta(line)
                if name is not None:
                    contigs.setdefault(n_contig if idx is None else idx, name)
                    n_contig += 1
            elif line.startswith(("##FILTER=<", "##INFO=<", "##FORMAT=<")):
                name, idx = _bcf_meta(line)
                if name is not None and name not in strings:
                    strings[name] = len(strings) if idx is None else idx
            elif line.startswith("#CHROM"):
                samples = [str(x) for x in line.split("\t")[9:]]
        if samples is None:
            raise ValueError('%s: the BCF header text has no #CHROM line' % path)
        return fh, contigs, strings.get("GT"), samples

    def _read(self, fh, number):
        head = fh.read(8)
        if not head:
            return None
        if len(head) < 8:
            raise ValueError("BCF: the file ends inside the lengths of record %d" % number)
        l_shared, l_indiv = struct.unpack("<II", head)
        body = fh.read(l_shared + l_indiv)
        if len(body) < l_shared + l_indiv:
            raise ValueError("BCF: record %d: the file ends inside it" % number)
        return BcfRecord(number, body[:l_shared], body[l_shared:], self._contigs, self._gt_key, len(self.samples))

    def __next__(self):
        self._number += 1
        rec = self._read(self._fh, self._number)
        if rec is None:
            raise StopIteration
        return rec

    def prepare(self, intervals):
        """One pass over the file for all the (contig, start, end) not looked up before: no index file is read."""
        import bisect
        todo = [iv for iv in dict.fromkeys(intervals) if iv not in self._indexed]
        if not todo:
            return
        by_contig = {}
        for iv in todo:
            self._indexed[iv] = []
            by_contig.setdefault(iv[0], []).append(iv)
        starts, longest = {}, {}
        for c, ivs in by_contig.items():
            ivs.sort(key=lambda iv: iv[1])
            starts[c] = [iv[1] for iv in ivs]
            longest[c] = max(iv[2] - iv[1] for iv in ivs)
        fh = self._open(self.path)[0]
        with fh:
            number = 0
            while True:
                number += 1
                rec = self._read(fh, number)
                if rec is None:
                    break
                if rec.contig not in by_contig:
                    continue
                a = rec.pos - 1
                b = a + len(rec.ref)
                ivs = by_contig[rec.contig]
                for j in range(bisect.bisect_left(starts[rec.contig], a - longest[rec.contig]), bisect.bisect_left(starts[rec.contig], b)):
                    if ivs[j][1] < b and a < ivs[j][2]:
                        self._indexed[ivs[j]].append(rec)


_REGION = re.compile(r'^(.+):(\d+)-(\d+)$')


def parse_region(region):
    """'contig:start-end' -> the (contig, start - 1, end) the reference hands to fetch (input.py:394-401), or None."""
    m = _REGION.match(region)
    return (m.group(1), int(m.group(2)) - 1, int(m.group(3))) if m else None


def open_variant_file(var_type, var_file, burden_file=None, burden_regions=None, uncompressed=False):
    """(handle, sample_order) (input.py:268-299)."""
    if var_type == "vcf":
        infile = BcfFile(var_file) if is_bcf(var_file) else VcfFile(var_file)
        if burden_file:
            load_burden(burden_file, burden_regions)
        return infile, []
    if var_type == "kmers":
        return (open(var_file) if uncompressed else gzip.open(var_file, 'r')), []
    if var_type == "Rtab":
        fh = open(var_file)
        header = fh.readline().rstrip()
        return fh, [str(x) for x in header.split()[1:]]
    raise ValueError('Variants type not supported (VCF input needs pysam, which this build does not ship)')


# ---------------------------------------------------------------------------------------------------------------
# per-variant parsing
# ---------------------------------------------------------------------------------------------------------------
def hash_pattern(k):
    """base64(md5(raw bytes of the presence vector)) + newline; the dtype of k matters (input.py:710-723)."""
    return binascii.b2a_base64(hashlib.md5(k.view(np.uint8)).digest())


def read_variant(infile, p, var_type, burden, burden_regions, uncompressed, all_strains, sample_order,
                 keep_list=None, noparse=False):
    """(eof, k, var_name, kstrains, nkstrains, af, missing) for the next line (input.py:301-454)."""
    if var_type not in ('kmers', 'vcf', 'Rtab'):
        raise ValueError('Variants type not supported')
    if var_type == "vcf":
        if burden:                                   # one variant per line of the regions file (input.py:355-361)
            line = burden_regions.popleft() if len(burden_regions) > 0 else None
        else:
            line = next(infile, None)
    else:
        line = infile.readline()
    if not line or noparse:
        return True, None, None, None, None, None, None
    d = {}
    if var_type == "vcf":
        if not burden:
            # (with a keep_list nothing of a record outside it is looked at, not even its ALT count: read_vcf_var, pyseer/input.py:473-478)
            if keep_list is not None and line.name_all_alleles() not in keep_list:
                return False, None, None, None, None, None, None
            var_name = infile.apply(line, d)
            if var_name is None:
                return False, None, None, None, None, None, None
        else:
            var_name, regions = line
            parsed = [parse_region(r) for r in regions]
            # the first look-up indexes this line's regions and all those still queued, in one pass over the file
            infile.prepare([r for r in parsed if r] + [r for r in (parse_region(x) for _, rs in burden_regions for x in rs) if r])
            for region in parsed:
                if region is None:
                    sys.stderr.write("Could not parse region %s\n" % str(region))      # (the reference prints its failed match: None)
                    continue
                for rec in infile.fetch(*region):
                    if keep_list is None or rec.name_all_alleles() in keep_list:      # (the reference hands the keep_list to the records of a region too)
                        infile.apply(rec, d)
    elif var_type == "kmers":
        if not uncompressed:
            line = line.decode()
        var_name = line.split()[0]
        strains = line.rstrip().split('|')[1].lstrip().split()
        if keep_list is not None and var_name not in keep_list:
            return False, None, None, None, None, None, None
        d = {str(x.split(':')[0]): 1 for x in strains}
    else:
        try:
            fields = line.rstrip().split('\t')
        except TypeError:
            fields = line.decode().rstrip().split('\t')
        var_name, calls = fields[0], fields[1:]
        if keep_list is not None and var_name not in keep_list:
            return False, None, None, None, None, None, None
        if len(calls) == 0:
            raise ValueError('No sample data found; is this a Rtab file?')
        if len(calls) != len(sample_order):
            raise ValueError('Unexpected mismatch between header and data row')
        for present, sample in zip(calls, sample_order):
            if present not in ('0', '1', '.', ''):
                raise ValueError('Rtab file not binary')
            if present == '1':
                d[sample] = 1
            elif present in ('.', ''):
                d[sample] = np.nan
    kstrains = sorted(set(d.keys()).intersection(all_strains))        # missing calls count as present here
    nkstrains = sorted(all_strains.difference(set(kstrains)))
    for x in nkstrains:
        d[x] = 0
    af = float(len(kstrains)) / len(all_strains)
    if len(kstrains) == 0:
        sys.stderr.write("No observations of " + var_name + " in selected samples\n")
    k = np.array([d[x] for x in p.index if x in d])
    missing = float(np.sum(np.isnan(k))) / len(all_strains)
    return False, k, var_name, kstrains, nkstrains, af, missing


def iter_variants(p, m, cov, var_type, burden, burden_regions, infile, all_strains, sample_order, lineage_effects,
                  lineage_clusters, min_af, max_af, max_missing, filter_pvalue, lrt_pvalue, null_fit, firth_null,
                  uncompressed, continuous):
    """Generator of fixed_effects_regression argument tuples (input.py:505-620); p slot is None for AF/missing-filtered."""
    while True:
        eof, k, var_name, kstrains, nkstrains, af, missing = read_variant(infile, p, var_type, burden, burden_regions,
                                                                          uncompressed, all_strains, sample_order)
        if eof:
            return
        pattern = hash_pattern(k) if k is not None else None
        keep = (k is not None) and (min_af <= af <= max_af) and not (missing > max_missing)
        yield (var_name, p.values if keep else None, k, m, cov.values, af, pattern, lineage_effects, lineage_clusters,
               filter_pvalue, lrt_pvalue, null_fit, firth_null, kstrains, nkstrains, continuous)


def load_var_block(var_type, p, burden, burden_regions, infile, all_strains, sample_order, min_af, max_af, max_missing,
                   uncompressed, block_size):
    """Generator of (variants, variant_mat, eof) blocks for the LMM (input.py:638-707)."""
    while True:
        variants = []
        variant_mat = np.zeros((len(p), block_size))
        eof = False
        for var_idx in range(block_size):
            eof, k, var_name, kstrains, nkstrains, af, missing = read_variant(infile, p, var_type, burden, burden_regions,
                                                                              uncompressed, all_strains, sample_order)
            if eof:
                break
            if k is None or af < min_af or af > max_af or missing > max_missing:
                pattern = None
            else:
                pattern = hash_pattern(k)
                variant_mat[:, var_idx] = k
            variants.append((var_obj.LMM(var_name, pattern, af, np.nan, np.nan, np.nan, np.nan, np.nan, np.nan, kstrains,
                                         nkstrains, set(), True, True), p.values, k))
        yield (variants, variant_mat, eof)
        if eof:
            break
    yield None, None, True


def iter_variants_lmm(variant_iter, lmm, h2, lineage, lineage_clusters, covariates, continuous, filter_pvalue, lrt_pvalue):
    """input.py:623-635"""
    for variants, variant_mat, eof in variant_iter:
        if len(variants) == 0:
            break
        yield (lmm, h2, variants, variant_mat, lineage, lineage_clusters, covariates, continuous, filter_pvalue, lrt_pvalue)
        if eof:
            break


# ---------------------------------------------------------------------------------------------------------------
# GPU feed
# ---------------------------------------------------------------------------------------------------------------
class PackedBlock(object):
    """One block of parsed variants: metadata lists + packed presence rows for those that reach the engine."""
    __slots__ = ("_names", "patterns", "afs", "kstrains", "nkstrains", "status", "bits", "row_of", "ks", "last_k",
                 "names_blob", "name_off")

    def __init__(self, n_samples, capacity):
        self._names, self.patterns, self.afs, self.kstrains, self.nkstrains = [], [], [], [], []
        self.status = []            # 0 = to engine, 1 = af/missing filtered, 2 = carries missing calls (NaN in k),
                                    # 3 = a VCF record the reader skipped (multi-allelic / FILTER): counted as loaded and pre-filtered, never a row
        self.ks = []                # the dense k only for status 2 (host-side handling of the error path)
        self.row_of = []            # row in self.bits, or -1
        self.names_blob = self.name_off = None     # concatenated names + offsets when the native reader supplied them
        self.last_k = None          # dense k of the LAST variant parsed into the block (see __main__: lmm.py:209-213)
        self.bits = np.zeros((capacity, row_bytes_for(n_samples)), dtype=np.uint8)

    @property
    def names(self):
        """Variant names as a list of str; decoded from the name blob only when somebody asks (the block sink does not)."""
        if self._names is None:
            b, o = self.names_blob, self.name_off
            self._names = [b[o[i]:o[i + 1]].decode() for i in range(len(o) - 1)]
        return self._names

    @names.setter
    def names(self, v):
        self._names = v

    def __len__(self):
        return len(self.status)


def iter_packed_blocks(p, var_type, infile, all_strains, sample_order, min_af, max_af, max_missing, uncompressed,
                       block_size, want_patterns=True, burden=False, burden_regions=None):
    """Parse `block_size` variants at a time into a PackedBlock (same filters as iter_variants / load_var_block)."""
    n = len(p)
    while True:
        blk = PackedBlock(n, block_size)
        nrow = 0
        eof = False
        for _ in range(block_size):
            eof, k, name, ks, nks, af, missing = read_variant(infile, p, var_type, burden, burden_regions, uncompressed, all_strains,
                                                              sample_order)
            if eof:
                break
            blk.last_k = k
            if name is None:                     # a skipped VCF record (input.py:608, :693: `k is None`)
                blk.names.append(''); blk.afs.append(np.nan); blk.kstrains.append(_NO_STRAINS); blk.nkstrains.append(_NO_STRAINS)
                blk.patterns.append(None); blk.status.append(3); blk.row_of.append(-1); blk.ks.append(None)
                continue
            blk.names.append(name); blk.afs.append(af); blk.kstrains.append(ks); blk.nkstrains.append(nks)
            if k is None or not (min_af <= af <= max_af) or missing > max_missing:
                blk.patterns.append(hash_pattern(k) if k is not None else None)
                blk.status.append(1); blk.row_of.append(-1); blk.ks.append(None)
                continue
            blk.patterns.append(hash_pattern(k) if want_patterns else b'')
            if missing > 0:
                blk.status.append(2); blk.row_of.append(-1); blk.ks.append(k)
                continue
            packed = np.packbits(k.astype(bool), bitorder="little")
            blk.bits[nrow, :packed.shape[0]] = packed
            blk.status.append(0); blk.row_of.append(nrow); blk.ks.append(None)
            nrow += 1
        blk.bits = blk.bits[:nrow]
        if blk.names:
            yield blk
        if eof:
            return


class NativeKmerReader(object):
    """Blocks of packed k-mer presence rows straight from the text file through libseerhip's reader (csrc/reader.cpp):
    gzip inflate + tokenise + sample lookup + bit packing in C++ (OpenMP over the lines of a block).  No GPU needed.
    engine: an Engine selects the device route (sh_reader_open_dev): the same containers, framing and names on the host, the sample tokens
    read by k_kmer_pack on the engine's device, on a stream of the reader's own.  DEVICE_HOST_RULE instead of an engine selects the
    library's host restatement of that kernel (checks without a device).  The blocks are the same arrays either way.
    inflate (device route only): True has the members of a BGZF file decoded by k_bgzf_inflate on the engine's device (DEVICE_HOST_RULE: by the
    host build of the same decoder), False never, None as SEERHIP_ROUTE kmer_inflate says; other containers are read as without it."""
    DEVICE_HOST_RULE = "device-route-host-rule"

    def __init__(self, path, sample_names, block_size=3000, max_name=256, engine=None, inflate=None):
        import ctypes as C
        from . import _abi
        self._C, self._abi = C, _abi
        self._lib = _abi.load()
        self.samples = [str(x) for x in sample_names]
        self.n = len(self.samples)
        arr = (C.c_char_p * self.n)(*[x.encode() for x in self.samples])
        self._engine = engine if engine is not None and engine != self.DEVICE_HOST_RULE else None      # (kept alive: the reader holds its context)
        self.device_route = engine is not None
        if engine is None:
            h = self._lib.sh_reader_open(str(path).encode(), arr, self.n)
        else:
            if inflate is not None:                         # (for this thread's next open only; the environment is not touched)
                self._lib.sh_reader_set_inflate(1 if inflate else 0)
            h = self._lib.sh_reader_open_dev(self._engine._h if self._engine is not None else None, str(path).encode(), arr, self.n)
        if not h:
            raise IOError(self._lib.sh_reader_error().decode())
        self._h = C.c_void_p(h)
        self.block_size = int(block_size)
        self.row_bytes = row_bytes_for(self.n)
        self._names = C.create_string_buffer(self.block_size * max_name)
        self._off = np.zeros(self.block_size + 1, dtype=np.int64)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.sh_reader_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def dev_stats(self):
        """The device route's counters (sh_reader_dev_stats): lines tokenised by the kernel / by the host restatement, text bytes sent to the
        device, kernel launches, and the kernel's own time in ms."""
        C = self._C
        a, b, c, d = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._abi.check(self._lib.sh_reader_dev_stats(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return {"lines_dev": a.value, "lines_host": b.value, "bytes_up": c.value, "launches": d.value,
                "kernel_ms": float(self._lib.sh_reader_dev_kernel_ms(self._h))}

    def inflate_stats(self):
        """The device inflate's counters (sh_reader_dev_inflate_stats): BGZF members decoded by the kernel (DEVICE_HOST_RULE: by the host build of
        its decoder) / decoded again by the host decoder, bytes sent up and brought back, and the kernel's own time in ms.  All zero where
        the route is off or the file is not BGZF."""
        C = self._C
        a, b, c, d, ms = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_double(0.0)
        self._abi.check(self._lib.sh_reader_dev_inflate_stats(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d), C.byref(ms)))
        return {"members_dev": a.value, "members_host": b.value, "bytes_up": c.value, "bytes_down": d.value, "kernel_ms": ms.value}

    def raw_blocks(self):
        """(bits, counts, names_blob, name_off) per block; names stay one bytes blob + offsets (what the block sink consumes)."""
        C, abi = self._C, self._abi
        while True:
            bits = np.zeros((self.block_size, self.row_bytes), dtype=np.uint8)
            counts = np.zeros(self.block_size, dtype=np.int32)
            nv = self._lib.sh_reader_next(self._h, self.block_size, bits.ctypes.data_as(abi.c_u8p), self.row_bytes,
                                          counts.ctypes.data_as(C.POINTER(C.c_int32)), self._names, len(self._names),
                                          self._off.ctypes.data_as(C.POINTER(C.c_int64)))
            if nv == -2:                                   # long names (unitigs): nothing was consumed, retry with room for them
                self._names = C.create_string_buffer(int(self._lib.sh_reader_names_needed(self._h)) * 2 + 1024)
                continue
            if nv < 0:
                raise IOError(self._lib.sh_reader_error().decode())
            if nv == 0:
                return
            yield bits[:nv], counts[:nv], self._names.raw[:self._off[nv]], self._off[:nv + 1].copy()

    def __iter__(self):
        """(names, bits, counts) per block, names decoded to str."""
        for bits, counts, blob, off in self.raw_blocks():
            yield [blob[off[v]:off[v + 1]].decode() for v in range(counts.shape[0])], bits, counts


class NativeVcfReader(object):
    """Blocks of VCF records through libseerhip's reader (sh_vcf_*: csrc/vcf_reader.cpp on the host, k_vcf_gt_pack on the device): per record
    the name, the skip reason, POS, len(REF), the contig and the packed present / missing rows over `sample_names`.
    engine: the Engine whose device and stream the reader uses; None selects the library's host restatement of the kernel (measurements and
    checks without a device -- the command line always passes its engine)."""

    def __init__(self, path, sample_names, engine=None, block_size=3000):
        import ctypes as C
        from . import _abi
        self._C, self._abi = C, _abi
        self._lib = _abi.load()
        self.samples = [str(x) for x in sample_names]
        self.n = len(self.samples)
        self._engine = engine                               # (kept alive: the reader holds its context)
        arr = (C.c_char_p * self.n)(*[x.encode() for x in self.samples])
        h = self._lib.sh_vcf_open(engine._h if engine is not None else None, str(path).encode(), arr, self.n)
        if not h:
            raise IOError(self._lib.sh_last_error().decode())
        self._h = C.c_void_p(h)
        self.block_size = int(block_size)
        self.row_bytes = row_bytes_for(self.n)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.sh_vcf_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        C = self._C
        mode, ncols, ncontigs = C.c_int(0), C.c_int(0), C.c_int(0)
        self._abi.check(self._lib.sh_vcf_info(self._h, C.byref(mode), C.byref(ncols), C.byref(ncontigs)))
        d = {"container": ("plain", "gzip", "bgzf")[mode.value], "columns": ncols.value, "contigs": ncontigs.value}
        if self.format != "vcf":                            # (a text file's dictionary stays what it was before BCF was read)
            d["format"] = self.format
        return d

    @property
    def format(self):
        """'vcf' or 'bcf': what the decoded bytes hold (sh_vcf_format), whatever the file is called."""
        return ("vcf", "bcf")[self._lib.sh_vcf_format(self._h)]

    def stats(self):
        C = self._C
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._abi.check(self._lib.sh_vcf_stats(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"sample_bytes": a.value, "records": b.value, "launches": c.value}

    def contig(self, i):
        return self._lib.sh_vcf_contig(self._h, int(i)).decode()

    def raw_blocks(self):
        """dict per block: blob / off (names), skip, pos, ref_len, contig, present, missing (packed rows), n_present, n_missing."""
        C = self._C
        i32, i64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        bs = self.block_size
        while True:
            skip = np.zeros(bs, dtype=np.int32); pos = np.zeros(bs, dtype=np.int64); ref_len = np.zeros(bs, dtype=np.int32)
            contig = np.zeros(bs, dtype=np.int32); n_p = np.zeros(bs, dtype=np.int32); n_m = np.zeros(bs, dtype=np.int32)
            present = np.zeros((bs, self.row_bytes), dtype=np.uint8); missing = np.zeros((bs, self.row_bytes), dtype=np.uint8)
            nv = self._lib.sh_vcf_next(self._h, bs, skip.ctypes.data_as(i32), pos.ctypes.data_as(i64), ref_len.ctypes.data_as(i32),
                                       contig.ctypes.data_as(i32), present.ctypes.data_as(self._abi.c_u8p), missing.ctypes.data_as(self._abi.c_u8p),
                                       self.row_bytes, n_p.ctypes.data_as(i32), n_m.ctypes.data_as(i32))
            if nv < 0:
                raise IOError(self._lib.sh_last_error().decode())
            if nv == 0:
                return
            blob_p, off_p = C.c_void_p(0), C.c_void_p(0)
            nb = self._lib.sh_vcf_names(self._h, C.byref(blob_p), C.byref(off_p))
            blob = C.string_at(blob_p.value, nb) if nb > 0 else b""
            off = np.frombuffer(C.string_at(off_p.value, 8 * (nv + 1)), dtype=np.int64).copy()
            yield {"blob": blob, "off": off, "skip": skip[:nv], "pos": pos[:nv], "ref_len": ref_len[:nv], "contig": contig[:nv],
                   "present": present[:nv], "missing": missing[:nv], "n_present": n_p[:nv], "n_missing": n_m[:nv]}


def _vcf_packed_block(n, samples, order, names, skip, present, missing, n_present, n_missing, min_af, max_af, max_missing, want_patterns,
                      messages=None):
    """The PackedBlock iter_packed_blocks builds from read_variant's tuples, from the native reader's rows instead: same names, af, sample
    lists, statuses, dense k for rows with missing calls, patterns, and the same lines on stderr in the same order.
    messages[i]: lines to write before record i's own (burden: what applying its regions said)."""
    nv = len(names)
    blk = PackedBlock(n, 0)
    dense_p = np.unpackbits(present, axis=1, bitorder="little")[:, :n]
    dense_m = np.unpackbits(missing, axis=1, bitorder="little")[:, :n]
    rows = []
    for i in range(nv):
        if messages is not None:
            sys.stderr.write(messages[i])
        if skip[i]:
            blk.last_k = None
            blk.names.append(''); blk.afs.append(np.nan); blk.kstrains.append(_NO_STRAINS); blk.nkstrains.append(_NO_STRAINS)
            blk.patterns.append(None); blk.status.append(3); blk.row_of.append(-1); blk.ks.append(None)
            continue
        nm = int(n_missing[i])
        cnt = int(n_present[i]) + nm
        af, miss = float(cnt) / n, float(nm) / n
        if cnt == 0:
            sys.stderr.write("No observations of " + names[i] + " in selected samples\n")
        carried = (dense_p[i] | dense_m[i]).astype(bool)
        ks = [samples[j] for j in order if carried[j]]
        nks = [samples[j] for j in order if not carried[j]]
        if nm:
            k = dense_p[i].astype(np.float64)
            k[dense_m[i].astype(bool)] = np.nan
        else:
            k = dense_p[i].astype(np.int64)
        blk.last_k = k
        blk.names.append(names[i]); blk.afs.append(af); blk.kstrains.append(ks); blk.nkstrains.append(nks)
        if not (min_af <= af <= max_af) or miss > max_missing:
            blk.patterns.append(hash_pattern(k)); blk.status.append(1); blk.row_of.append(-1); blk.ks.append(None)
            continue
        blk.patterns.append(hash_pattern(k) if want_patterns else b'')
        if nm:
            blk.status.append(2); blk.row_of.append(-1); blk.ks.append(k)
            continue
        blk.status.append(0); blk.row_of.append(len(rows)); blk.ks.append(None)
        rows.append(i)
    blk.bits = np.ascontiguousarray(present[rows]) if rows else np.zeros((0, present.shape[1]), dtype=np.uint8)
    return blk


def _merged_intervals(regions):
    """{contig: (starts, ends)} of the union of the (contig, start, end) given, as sorted disjoint intervals."""
    by = {}
    for c, s_, e_ in regions:
        by.setdefault(c, []).append((s_, e_))
    out = {}
    for c, ivs in by.items():
        ivs.sort()
        merged = [list(ivs[0])]
        for s_, e_ in ivs[1:]:
            if s_ <= merged[-1][1]:
                merged[-1][1] = max(merged[-1][1], e_)
            else:
                merged.append([s_, e_])
        out[c] = (np.array([m_[0] for m_ in merged], dtype=np.int64), np.array([m_[1] for m_ in merged], dtype=np.int64))
    return out


class CallBlock(object):
    """One block of variants with missing calls as the native VCF reader (or k_burden_fold over its rows) delivers them, every variant in
    input order and BEFORE any AF window: names (blob / off, `names` decodes them), the reader's skip reason, the packed present / missing
    rows with their counts, and per variant the text read_variant writes to stderr while it applies its records ("Multiple alleles at ...
    Skipping", "Could not parse region None"; "" for most)."""
    __slots__ = ("blob", "off", "skip", "present", "missing", "n_present", "n_missing", "messages", "_names", "msg_rows")

    def __init__(self, blob, off, skip, present, missing, n_present, n_missing, messages, msg_rows=None):
        """msg_rows: the indices of the variants whose message is not empty, where the producer knows them (None: look)"""
        self.blob, self.off, self.skip, self.present, self.missing = blob, off, skip, present, missing
        self.n_present, self.n_missing, self.messages, self._names, self.msg_rows = n_present, n_missing, messages, None, msg_rows

    def __len__(self):
        return int(self.skip.shape[0])

    @property
    def names(self):
        if self._names is None:
            blob, off = self.blob, self.off
            self._names = [blob[off[i]:off[i + 1]].decode() for i in range(len(off) - 1)]
        return self._names


def _multi_message(contig, pos):
    return "Multiple alleles at %s_%d. Skipping\n" % (contig, pos)


def _vcf_call_blocks(reader, engine, block_size, burden_regions=None):
    """The CallBlock stream behind iter_packed_blocks_vcf_native and iter_call_blocks_vcf_native: one variant per record, or, with
    burden_regions (the (name, [region, ...]) list load_burden fills), one per entry: the file is read once, the rows of the records that lie
    in any region are kept, and k_burden_fold (sh_burden_fold) combines each variant's records on the device."""
    def plain():
        for rb in reader.raw_blocks():
            nv = rb["skip"].shape[0]
            msgs = [""] * nv
            multi = np.nonzero(rb["skip"] == VCF_MULTI)[0]
            for i in multi:
                msgs[i] = _multi_message(reader.contig(rb["contig"][i]), int(rb["pos"][i]))
            yield CallBlock(rb["blob"], rb["off"], rb["skip"], rb["present"], rb["missing"], rb["n_present"], rb["n_missing"], msgs, multi)

    def burden():
        import ctypes as C
        from . import _abi
        variants = list(burden_regions)
        parsed = [[parse_region(r) for r in regions] for _, regions in variants]
        union = _merged_intervals([r for rs in parsed for r in rs if r])
        # pass over the file: the records that meet any region stay (rows, span, skip reason), the rest are dropped
        keep = {"contig": [], "a": [], "b": [], "skip": [], "present": [], "missing": []}
        for rb in reader.raw_blocks():
            a = rb["pos"] - 1
            b = a + rb["ref_len"]
            hit = np.zeros(a.shape[0], dtype=bool)
            for cid in np.unique(rb["contig"]):
                iv = union.get(reader.contig(cid))
                if iv is None:
                    continue
                sel = rb["contig"] == cid
                j = np.searchsorted(iv[0], b[sel], side="left") - 1             # the last interval that starts before the record ends
                hit[sel] = (j >= 0) & (a[sel] < iv[1][np.maximum(j, 0)])
            if hit.any():
                keep["contig"].append(np.array([reader.contig(c) for c in rb["contig"][hit]], dtype=object))
                keep["a"].append(a[hit]); keep["b"].append(b[hit]); keep["skip"].append(rb["skip"][hit])
                keep["present"].append(rb["present"][hit]); keep["missing"].append(rb["missing"][hit])
        rb_ = reader.row_bytes
        if keep["a"]:
            kc = np.concatenate(keep["contig"]); ka = np.concatenate(keep["a"]); kb = np.concatenate(keep["b"]); ksk = np.concatenate(keep["skip"])
            kp = np.ascontiguousarray(np.concatenate(keep["present"])); km = np.ascontiguousarray(np.concatenate(keep["missing"]))
        else:
            kc = np.zeros(0, dtype=object); ka = kb = np.zeros(0, dtype=np.int64); ksk = np.zeros(0, dtype=np.int32)
            kp = km = np.zeros((0, rb_), dtype=np.uint8)
        by_contig = {}
        for c in set(kc.tolist()):
            idx = np.nonzero(kc == c)[0]
            o = np.argsort(ka[idx], kind="stable")
            by_contig[c] = (idx[o], ka[idx][o], int((kb[idx] - ka[idx]).max()))
        lib = _abi.load()
        i32, i64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        for v0 in range(0, len(variants), block_size):
            chunk = range(v0, min(len(variants), v0 + block_size))
            msgs, csr_off, csr_idx = [], [0], []
            for v in chunk:
                msg = ""
                for region in parsed[v]:
                    if region is None:
                        msg += "Could not parse region %s\n" % str(region)
                        continue
                    contig, start, end = region
                    if contig not in by_contig:
                        continue
                    idx, a_sorted, longest = by_contig[contig]
                    cand = idx[np.searchsorted(a_sorted, start - longest, side="left"):np.searchsorted(a_sorted, end, side="left")]
                    cand = np.sort(cand[kb[cand] > start])                   # file order
                    for rec in cand:
                        if ksk[rec] == VCF_MULTI:
                            msg += _multi_message(contig, int(ka[rec]) + 1)
                        if ksk[rec] == VCF_KEPT:
                            csr_idx.append(int(rec))
                msgs.append(msg)
                csr_off.append(len(csr_idx))
            nvar = len(chunk)
            off_a = np.array(csr_off, dtype=np.int64); idx_a = np.array(csr_idx if csr_idx else [0], dtype=np.int32)
            out_p = np.zeros((nvar, rb_), dtype=np.uint8); out_m = np.zeros((nvar, rb_), dtype=np.uint8)
            n_p = np.zeros(nvar, dtype=np.int32); n_m = np.zeros(nvar, dtype=np.int32)
            if engine is None:
                raise ValueError("burden regions need the device (sh_burden_fold)")
            _abi.check(lib.sh_burden_fold(engine._h, kp.ctypes.data_as(_abi.c_u8p), km.ctypes.data_as(_abi.c_u8p), rb_, kp.shape[0], off_a.ctypes.data_as(i64),
                                          idx_a.ctypes.data_as(i32), nvar, out_p.ctypes.data_as(_abi.c_u8p), out_m.ctypes.data_as(_abi.c_u8p),
                                          n_p.ctypes.data_as(i32), n_m.ctypes.data_as(i32)))
            enc = [variants[v][0].encode() for v in chunk]
            off_n = np.zeros(nvar + 1, dtype=np.int64)
            np.cumsum([len(x) for x in enc], out=off_n[1:])
            blk = CallBlock(b"".join(enc), off_n, np.zeros(nvar, dtype=np.int32), out_p, out_m, n_p, n_m, msgs,
                            np.array([i for i, m_ in enumerate(msgs) if m_], dtype=np.int64))
            blk._names = [variants[v][0] for v in chunk]
            yield blk

    return burden() if burden_regions is not None else plain()


def iter_packed_blocks_vcf_native(p, path, engine, min_af, max_af, max_missing, block_size, want_patterns=True, burden_regions=None, save_to=None):
    """The PackedBlock stream of iter_packed_blocks(p, 'vcf', ...) fed by the native reader (_vcf_call_blocks; burden_regions: one variant per
    entry of the (name, [region, ...]) list load_burden fills).  save_to: a CallCacheWriter that takes every CallBlock as read (--save-calls)."""
    samples = [str(x) for x in p.index]
    order = sorted(range(len(samples)), key=lambda i: samples[i])
    n = len(samples)
    reader = NativeVcfReader(path, samples, engine, block_size)
    try:
        for cb in _vcf_call_blocks(reader, engine, block_size, burden_regions):
            if save_to is not None:
                save_to.write(cb)
            yield _vcf_packed_block(n, samples, order, cb.names, cb.skip, cb.present, cb.missing, cb.n_present, cb.n_missing,
                                    min_af, max_af, max_missing, want_patterns, cb.messages)
    finally:
        reader.close()


def iter_call_blocks_vcf_native(p, path, engine, block_size, burden_regions=None):
    """The CallBlock stream of a VCF for the whole-genome models (enet.load_all_vars_calls): every record in input order, or one variant per
    line of the regions file, before any AF window -- the filter, the coding and the storing are the device's (sh_enet_ingest_calls)."""
    reader = NativeVcfReader(path, [str(x) for x in p.index], engine, block_size)
    try:
        for cb in _vcf_call_blocks(reader, engine, block_size, burden_regions):
            yield cb
    finally:
        reader.close()


RTAB_ERRORS = {1: 'No sample data found; is this a Rtab file?',            # row status of sh_rtab_next -> read_variant's ValueError (input.py:377-383)
               2: 'Unexpected mismatch between header and data row',
               3: 'Rtab file not binary'}
LAST_RTAB_LAUNCHES = None     # kernel launches (sh_rtab_stats) of the last native Rtab reader this process closed; None: none was opened


class RtabDuplicateSample(ValueError):
    """The header names a phenotype sample in more than one column: sh_rtab_open refuses, the callers read the table line by line."""


class NativeRtabReader(object):
    """Blocks of Rtab lines through libseerhip's reader (sh_rtab_*: csrc/rtab_reader.cpp on the host, k_rtab_pack on the device): per line the
    name, a status (0 ok, else a key of RTAB_ERRORS; such a line has rows of zeros) and the packed present / missing rows over `sample_names`.
    The header is split here, with the reference's own expression, and handed to the library, which skips the first line.
    engine: the Engine whose device and stream the reader uses; None selects the library's host restatement of the kernel.
    Raises RtabDuplicateSample when two columns name the same phenotype sample: the reference lets the last call that is not `0` win there,
    which no OR of bits reproduces, so every caller in this package then takes the Python reader (read_variant) and prints the same bytes."""

    def __init__(self, path, sample_names, engine=None, block_size=3000):
        import ctypes as C
        from . import _abi
        self._C, self._abi = C, _abi
        self._lib = _abi.load()
        self.samples = [str(x) for x in sample_names]
        self.n = len(self.samples)
        self._engine = engine                               # (kept alive: the reader holds its context)
        with open(path) as fh:
            header = fh.readline().rstrip()
        self.columns = [str(x) for x in header.split()[1:]]
        arr = (C.c_char_p * self.n)(*[x.encode() for x in self.samples])
        cols = (C.c_char_p * max(1, len(self.columns)))(*[x.encode() for x in self.columns])
        h = self._lib.sh_rtab_open(engine._h if engine is not None else None, str(path).encode(), arr, self.n, cols, len(self.columns))
        if not h:
            msg = self._lib.sh_last_error().decode()
            if msg.startswith("Rtab: duplicate sample column"):
                raise RtabDuplicateSample(msg)
            raise IOError(msg)
        self._h = C.c_void_p(h)
        self.block_size = int(block_size)
        self.row_bytes = row_bytes_for(self.n)

    def close(self):
        global LAST_RTAB_LAUNCHES
        if getattr(self, "_h", None):
            LAST_RTAB_LAUNCHES = self.stats()["launches"]
            self._lib.sh_rtab_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def stats(self):
        C = self._C
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._abi.check(self._lib.sh_rtab_stats(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"call_bytes": a.value, "rows": b.value, "launches": c.value}

    def partition(self):
        """Bytes of call text per lane, per wavefront and per step of k_rtab_pack as this reader launches it."""
        C = self._C
        a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
        self._abi.check(self._lib.sh_rtab_partition(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"lane": a.value, "wave": b.value, "step": c.value}

    def raw_blocks(self):
        """dict per block: blob / off (names), status, skip (zeros), present, missing (packed rows), n_present, n_missing."""
        C = self._C
        i32 = C.POINTER(C.c_int32)
        bs = self.block_size
        while True:
            status = np.zeros(bs, dtype=np.int32); n_p = np.zeros(bs, dtype=np.int32); n_m = np.zeros(bs, dtype=np.int32)
            present = np.zeros((bs, self.row_bytes), dtype=np.uint8); missing = np.zeros((bs, self.row_bytes), dtype=np.uint8)
            nv = self._lib.sh_rtab_next(self._h, bs, status.ctypes.data_as(i32), present.ctypes.data_as(self._abi.c_u8p),
                                        missing.ctypes.data_as(self._abi.c_u8p), self.row_bytes, n_p.ctypes.data_as(i32), n_m.ctypes.data_as(i32))
            if nv < 0:
                raise IOError(self._lib.sh_last_error().decode())
            if nv == 0:
                return
            blob_p, off_p = C.c_void_p(0), C.c_void_p(0)
            nb = self._lib.sh_rtab_names(self._h, C.byref(blob_p), C.byref(off_p))
            blob = C.string_at(blob_p.value, nb) if nb > 0 else b""
            off = np.frombuffer(C.string_at(off_p.value, 8 * (nv + 1)), dtype=np.int64).copy()
            yield {"blob": blob, "off": off, "status": status[:nv], "skip": np.zeros(nv, dtype=np.int32), "present": present[:nv],
                   "missing": missing[:nv], "n_present": n_p[:nv], "n_missing": n_m[:nv]}


def _rtab_call_blocks(reader):
    """(CallBlock, error) per block of the reader: error is None, or the ValueError of the block's first malformed line -- the block then
    holds only the lines before it, and is the last."""
    for rb in reader.raw_blocks():
        bad = np.nonzero(rb["status"])[0]
        nv = int(bad[0]) if bad.size else rb["status"].shape[0]
        cb = CallBlock(rb["blob"][:rb["off"][nv]], rb["off"][:nv + 1], rb["skip"][:nv], rb["present"][:nv], rb["missing"][:nv], rb["n_present"][:nv],
                       rb["n_missing"][:nv], [""] * nv, np.zeros(0, dtype=np.int64))
        yield cb, (ValueError(RTAB_ERRORS[int(rb["status"][nv])]) if bad.size else None)
        if bad.size:
            return


def iter_packed_blocks_rtab_native(p, path, engine, min_af, max_af, max_missing, block_size, want_patterns=True, save_to=None):
    """The PackedBlock stream of iter_packed_blocks(p, 'Rtab', ...) fed by the native reader: same names, af (present + missing over n), sample
    lists, statuses, dense k for rows with missing calls, patterns and stderr lines.  A malformed line raises read_variant's ValueError once
    every complete block before it has been yielded and the lines before it in its own block have said what read_variant says of them -- the
    point at which the line-by-line route raises.  A header that names a phenotype sample twice: the line-by-line route itself."""
    samples = [str(x) for x in p.index]
    order = sorted(range(len(samples)), key=lambda i: samples[i])
    n = len(samples)
    try:
        reader = NativeRtabReader(path, samples, engine, block_size)
    except RtabDuplicateSample:
        infile, sample_order = open_variant_file("Rtab", path)
        for blk in iter_packed_blocks(p, "Rtab", infile, set(p.index), sample_order, min_af, max_af, max_missing, False, block_size, want_patterns=want_patterns):
            yield blk
        return
    try:
        for cb, error in _rtab_call_blocks(reader):
            if save_to is not None:                    # (--save-calls; a malformed line ends the run, and the run's end without close() leaves no cache)
                save_to.write(cb)
            blk = _vcf_packed_block(n, samples, order, cb.names, cb.skip, cb.present, cb.missing, cb.n_present, cb.n_missing,
                                    min_af, max_af, max_missing, want_patterns)
            if error is not None:
                raise error
            yield blk
    finally:
        reader.close()


def iter_call_blocks_rtab_native(p, path, engine, block_size):
    """The CallBlock stream of an Rtab for the whole-genome models (enet.load_all_vars_calls): every line in input order, before any AF window.
    A malformed line raises read_variant's ValueError after the lines before it have been yielded (a last, shorter block), so that the
    consumer has said of them what the line-by-line route says before it raises.  Not for a header that names a phenotype sample twice
    (RtabDuplicateSample: the caller keeps load_all_vars)."""
    reader = NativeRtabReader(path, [str(x) for x in p.index], engine, block_size)
    try:
        for cb, error in _rtab_call_blocks(reader):
            if len(cb):
                yield cb
            if error is not None:
                raise error
    finally:
        reader.close()


def say_call_block(cb):
    """What the default route (_vcf_packed_block) writes to stderr about a CallBlock, in its order: per variant the reader's own message, then
    "No observations of ..." for a variant nobody carries.  Only the variants that have something to say are visited."""
    quiet = (np.asarray(cb.skip) == 0) & ((np.asarray(cb.n_present) + np.asarray(cb.n_missing)) == 0)
    rows = cb.msg_rows if cb.msg_rows is not None else np.array([i for i, m_ in enumerate(cb.messages) if m_], dtype=np.int64)
    rows = np.union1d(np.asarray(rows, dtype=np.int64), np.nonzero(quiet)[0])
    if rows.shape[0]:
        blob, off = cb.blob, cb.off
        sys.stderr.write("".join(cb.messages[i] + ("No observations of " + bytes(blob[off[i]:off[i + 1]]).decode() + " in selected samples\n" if quiet[i] else "")
                                 for i in rows.tolist()))


def _job_call_block(cb):
    """The CallBlock as Job.submit_calls takes it: C-contiguous planes and int32 counts (views of the reader's arrays where they are that already)."""
    c = np.ascontiguousarray
    return CallBlock(cb.blob, c(cb.off, dtype=np.int64), c(cb.skip, dtype=np.int32), c(cb.present, dtype=np.uint8), c(cb.missing, dtype=np.uint8),
                     c(cb.n_present, dtype=np.int32), c(cb.n_missing, dtype=np.int32), cb.messages, cb.msg_rows)


def iter_job_call_blocks_vcf(p, path, engine, block_size, burden_regions=None, save_to=None):
    """The CallBlocks of a VCF / BCF (or of its burden regions) for the job stream (--device-calls: Job.submit_calls), as parsed: the stderr
    lines of the default route are written here, block by block, and nothing else is done per variant."""
    for cb in iter_call_blocks_vcf_native(p, path, engine, block_size, burden_regions):
        if save_to is not None:
            save_to.write(cb)
        say_call_block(cb)
        if len(cb):
            yield _job_call_block(cb)


def iter_job_call_blocks_rtab(reader, save_to=None):
    """The same for an Rtab through an open NativeRtabReader (closed here).  A malformed line raises read_variant's ValueError where the default
    route raises it: behind the stderr lines of the lines before it in its block."""
    try:
        for cb, error in _rtab_call_blocks(reader):
            if save_to is not None:
                save_to.write(cb)
            say_call_block(cb)
            if error is not None:
                raise error
            if len(cb):
                yield _job_call_block(cb)
    finally:
        reader.close()


def prefetched(iterable, depth=2):
    """Run `iterable` in a background thread, `depth` items ahead.  The native reader spends its time inside ctypes calls (GIL
    released: inflate + OpenMP parse), so block k+1 is read and packed while block k is on the GPU / being formatted."""
    import queue
    import threading
    q = queue.Queue(maxsize=depth)
    end = object()

    def work():
        try:
            for item in iterable:
                q.put((item, None))
        except BaseException as ex:           # re-raised in the consumer
            q.put((None, ex))
        q.put((end, None))

    t = threading.Thread(target=work, daemon=True)
    t.start()
    while True:
        item, ex = q.get()
        if ex is not None:
            raise ex
        if item is end:
            return
        yield item


def strains_from_bits(row, samples_sorted_idx, samples):
    """(kstrains, nkstrains), both lexicographically sorted like read_variant's (input.py:439-440), from one packed row."""
    present = np.unpackbits(row, bitorder="little")[:len(samples)].astype(bool)
    ks = [samples[i] for i in samples_sorted_idx if present[i]]
    nks = [samples[i] for i in samples_sorted_idx if not present[i]]
    return ks, nks


_NO_STRAINS = ()           # shared placeholder when the sample lists are not wanted (read-only)


class _Repeat(object):
    """n copies of one read-only value, indexable and iterable like the list it stands for (a block's per-row lists of placeholders were
    four 262 144-element lists per block, built while holding the GIL)."""
    __slots__ = ("v", "n")

    def __init__(self, v, n):
        self.v, self.n = v, int(n)

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self.v] * len(range(*i.indices(self.n)))
        if not -self.n <= i < self.n:
            raise IndexError(i)
        return self.v

    def __iter__(self):
        import itertools
        return itertools.repeat(self.v, self.n)


class RawBlock(object):
    """One block as the job stream takes it (engine.Job.submit): the parsed rows and nothing derived from them -- the AF window, the masks,
    the counters and the choice of the printed rows happen on the device.  dma: the rows may be read by the device where they lie
    (a registered window of the packed-cache mapping); release(): called once the block has been collected."""
    __slots__ = ("blob", "off", "counts", "bits", "dma", "release")

    def __init__(self, blob, off, counts, bits, dma=False, release=None):
        self.blob, self.off, self.counts, self.bits, self.dma, self.release = blob, off, counts, bits, dma, release

    def __len__(self):
        return int(self.counts.shape[0])


def _raw_block(blob, off, counts, bits, dma=False, release=None, say_empty=True):
    """say_empty=False: the consumer parses only some of the lines (enet_predict: those the model names) and says it for those itself."""
    off = np.require(off, dtype=np.int64, requirements=["A", "C"]); counts = np.require(counts, dtype=np.int32, requirements=["A", "C"])   # (views of a mapping may be misaligned)
    for i in (np.nonzero(counts == 0)[0] if say_empty else ()):   # (read_variant's message, pyseer/input.py:441-443)
        sys.stderr.write("No observations of " + bytes(blob[off[i]:off[i + 1]]).decode() + " in selected samples\n")
    return RawBlock(blob, off, counts, bits, dma, release)


def _block_from_raw(n, samples, order, names, blob, off, bits, counts, min_af, max_af, want_patterns, want_samples):
    """PackedBlock from one raw block of the native reader / the packed cache (all parsed variants, before the AF filter)."""
    blk = PackedBlock(n, 0)
    blk.names_blob, blk.name_off = blob, off
    afs = counts.astype(np.float64) / n
    keep = (afs >= min_af) & (afs <= max_af)
    blk.names = names                                    # None = decode lazily from the blob
    # arrays, not lists (round 3: 262 144-element .tolist() calls and their np.asarray() twins in the sink were a third of a block's
    # host time), and EVERY row goes to the engine in place: no compacted copy of the kept rows (170 MB per block at N = 5000).  The
    # driver sets the engine's own AF window (sh_set_af_filter: same inclusive bounds on count / n, input.py:608), so rows outside it
    # cost the GPU nothing; their statistics are masked by `status` in the sink either way.
    blk.afs = afs
    blk.status = np.where(keep, 0, 1).astype(np.int8)
    nv = int(counts.shape[0])
    blk.row_of = np.arange(nv, dtype=np.int64)
    blk.ks = _Repeat(None, nv)
    blk.bits = bits
    if want_samples:
        sp = [strains_from_bits(bits[i], order, samples) for i in range(nv)]
        blk.kstrains = [a for a, _ in sp]; blk.nkstrains = [b for _, b in sp]
    else:
        blk.kstrains = _Repeat(_NO_STRAINS, nv); blk.nkstrains = blk.kstrains
    if want_patterns:
        dense = np.unpackbits(bits, axis=1, bitorder="little")[:, :n].astype(np.int64)
        blk.patterns = [hash_pattern(dense[i]) for i in range(nv)]
    else:
        blk.patterns = _Repeat(b'', nv)
    for i in np.nonzero(counts == 0)[0]:
        sys.stderr.write("No observations of " + blob[off[i]:off[i + 1]].decode() + " in selected samples\n")
    blk.last_k = np.unpackbits(bits[nv - 1], bitorder="little")[:n].astype(np.int64)
    return blk


def iter_packed_blocks_native(p, path, min_af, max_af, block_size, want_patterns=False, want_samples=False, save_to=None, raw=False, say_empty=True,
                              engine=None, inflate=None):
    """Same PackedBlock stream as iter_packed_blocks for k-mer files, fed by the native reader.  save_to: a PackedCacheWriter that
    receives every raw block (all parsed variants, before the AF filter).  raw: RawBlock objects for the job stream instead.
    engine: the sample tokens are read on that engine's device (NativeKmerReader, --device-reader); the blocks are the same.
    inflate: with an engine, a BGZF file's members are decoded there too (--device-inflate); None: as SEERHIP_ROUTE kmer_inflate says."""
    samples = [str(x) for x in p.index]
    order = sorted(range(len(samples)), key=lambda i: samples[i])
    n = len(samples)
    reader = NativeKmerReader(path, samples, block_size, engine=engine, inflate=inflate)
    def finished():                      # the whole of a block's host preparation runs on the reader's thread, ahead of the engine
        for bits, counts, blob, off in reader.raw_blocks():
            if save_to is not None:
                save_to.write_block(blob, off, counts, bits)
            if raw:
                yield _raw_block(blob, off, counts, bits, say_empty=say_empty)
            else:
                yield _block_from_raw(n, samples, order, None, blob, off, bits, counts, min_af, max_af, want_patterns, want_samples)

    for blk in prefetched(finished()):
        yield blk


def iter_packed_blocks_native_multi(p, paths, min_af, max_af, block_size, want_patterns=False, want_samples=False,
                                    ahead_bytes=2 << 30, raw=False):
    """Several k-mer files as ONE stream, in the order given (`--kmers a.gz b.gz ...`), with all of them read at once.

    A single gzip stream inflates serially (38 k k-mers/s at N = 5000 on the GPU host, against tens of millions per second of
    compute), so the only way to feed the engine faster from gzip is more streams.  Every file gets its own native reader on its
    own thread, started immediately; what a reader produces are packed bit rows (N / 8 bytes per k-mer, ~40x smaller than the text),
    queued per file.  The consumer drains the queues in file order, so the output is what the concatenated file would give; while it
    works through the first file the others are parsed into their queues, each bounded by `ahead_bytes` of packed rows."""
    import queue
    import threading
    samples = [str(x) for x in p.index]
    order = sorted(range(len(samples)), key=lambda i: samples[i])
    n = len(samples)
    end = object()

    class Feed(object):
        def __init__(self, path):
            self.q = queue.Queue()
            self.room = threading.Semaphore(0)
            self.held = 0
            self.lock = threading.Lock()
            self.reader, self.open_error = None, None
            try:
                self.reader = NativeKmerReader(path, samples, block_size)
            except BaseException as ex:       # re-raised in the consumer, in file order
                self.open_error = ex
            self.t = threading.Thread(target=self.work, daemon=True)
            self.t.start()

        def work(self):
            try:
                if self.open_error is not None:
                    raise self.open_error
                for raw in self.reader.raw_blocks():
                    nb = int(raw[0].nbytes) + int(raw[2].nbytes if hasattr(raw[2], "nbytes") else len(raw[2]))
                    while True:
                        with self.lock:
                            if self.held == 0 or self.held + nb <= ahead_bytes:
                                self.held += nb
                                break
                        self.room.acquire()
                    self.q.put((raw, nb, None))
            except BaseException as ex:       # re-raised in the consumer
                self.q.put((None, 0, ex))
            self.q.put((end, 0, None))

        def blocks(self):
            while True:
                raw, nb, ex = self.q.get()
                if ex is not None:
                    raise ex
                if raw is end:
                    return
                with self.lock:
                    self.held -= nb
                self.room.release()
                yield raw

    # one look-ahead budget and one pool of parser threads for all the files (round 2 gave every file 2 GB and a full pool: 16 GB and ~380
    # threads for 8 files under a 16-CPU quota)
    ahead_bytes = max(64 << 20, int(ahead_bytes) // max(1, len(paths)))
    from . import _abi
    _abi.load().sh_reader_set_concurrency(len(paths))
    try:
        feeds = [Feed(path) for path in paths]                       # every reader is opened here, under the shared-pool hint
    finally:
        _abi.load().sh_reader_set_concurrency(1)
    for f in feeds:
        for bits, counts, blob, off in f.blocks():
            if raw:
                yield _raw_block(blob, off, counts, bits)
            else:
                yield _block_from_raw(n, samples, order, None, blob, off, bits, counts, min_af, max_af, want_patterns, want_samples)


# ---------------------------------------------------------------------------------------------------------------
# Packed cache: the parsed k-mer file as bit rows, so that further runs over the same samples (another phenotype column,
# other covariates, LMM after fixed effects) skip gzip and text parsing and stream at the engine's rate.  A run over a subset or another
# order of the stored samples reads it too: iter_packed_blocks_cached(select=), whose rows are selected on the device (k_rows_select).
#   header: b"SEERPK01", uint32 n_samples, uint32 row_bytes, uint64 len, sample names joined by "\n" (phenotype order)
#   blocks: uint64 nv, uint64 name_bytes, int64 name_off[nv+1], int32 counts[nv], names, uint8 bits[nv*row_bytes]; nv = 0 ends
# ---------------------------------------------------------------------------------------------------------------
_PK_MAGIC = b"SEERPK01"


class PackedCacheWriter(object):
    """Writes to `path + ".part"` and renames onto `path` in close(), after the terminator and an fsync: a run that is interrupted or fails
    leaves no `path` at all (round 2 wrote in place, and a truncated cache with a valid header was accepted by every later run until it
    died in the middle of its output).  `stamp` = (sidecar path, text): written only once the cache itself is in place."""

    def __init__(self, path, samples, stamp=None):
        self._path, self._tmp, self._stamp = path, path + ".part", stamp
        self._f = open(self._tmp, "wb")
        names = "\n".join(samples).encode()
        self._f.write(_PK_MAGIC + np.array([len(samples), row_bytes_for(len(samples))], dtype="<u4").tobytes()
                      + np.array([len(names)], dtype="<u8").tobytes() + names)

    def write_block(self, blob, off, counts, bits):
        nv = int(counts.shape[0])
        self._f.write(np.array([nv, len(blob)], dtype="<u8").tobytes())
        self._f.write(np.ascontiguousarray(off, dtype="<i8").tobytes())
        self._f.write(np.ascontiguousarray(counts, dtype="<i4").tobytes())
        self._f.write(blob)
        self._f.write(np.ascontiguousarray(bits, dtype=np.uint8).tobytes())

    def close(self):
        import os
        if self._f is not None:
            self._f.write(np.array([0, 0], dtype="<u8").tobytes())
            self._f.flush()
            os.fsync(self._f.fileno())
            self._f.close()
            self._f = None
            os.replace(self._tmp, self._path)
            if self._stamp is not None:
                with open(self._stamp[0], "w") as f:
                    f.write(self._stamp[1] + "\n")

    def abort(self):
        """Drop what was written (the run did not finish): no cache, no stamp."""
        import os
        if self._f is not None:
            self._f.close()
            self._f = None
            try:
                os.remove(self._tmp)
            except OSError:
                pass

    def __del__(self):
        try:
            self.abort()
        except Exception:
            pass


def packed_cache_complete(path):
    """True if `path` ends with the terminator close() writes (nv = 0, name_bytes = 0): a cheap test that the file was written to its end."""
    import os
    try:
        if os.path.getsize(path) < 8 + 8 + 8 + 16:
            return False
        with open(path, "rb") as f:
            f.seek(-16, 2)
            return f.read(16) == b"\0" * 16
    except (IOError, OSError):
        return False


# ---------------------------------------------------------------------------------------------------------------
# Call cache: the CallBlocks of a VCF / BCF (single records or burden regions) or an Rtab, so that further runs over the same samples, a subset
# or another order of them skip the text.  What does not depend on the run's samples is stored as read (names, skip, the readers' messages);
# the planes are stored over the cache's sample list and restricted to the run's when they are loaded (k_calls_select), where the two counts
# and the "No observations of ..." lines are made anew (say_call_block).
#   header: b"SEERCL01", uint32 n_samples, uint32 row_bytes, uint64 len, sample names joined by "\n", zeros up to a multiple of 8
#   blocks: uint64 nv, uint64 name_bytes, uint64 msg_bytes, uint64 0, int64 name_off[nv+1], int64 msg_off[nv+1], int32 skip[nv], int32 n_present[nv],
#           int32 n_missing[nv], names, messages, zeros up to a multiple of 8, uint8 present[nv*row_bytes], uint8 missing[nv*row_bytes]; nv = 0 ends
# Every block starts, and its planes start, on a multiple of 8 (row_bytes is one): a mapped plane can be read as 64-bit words.
# ---------------------------------------------------------------------------------------------------------------
_CL_MAGIC = b"SEERCL01"


def _pad8(n):
    return (-n) % 8


class CallCacheWriter(object):
    """CallBlocks in, re-cut into stored blocks of `block_rows` variants (a loader never splits a stored block: block_rows is the --block_size
    of the runs the cache is for).  Written to `path + ".part"`, ended by a terminator, fsynced and renamed in close(), as PackedCacheWriter:
    a run that fails or is interrupted (abort(), or no close() at all) leaves no cache."""

    def __init__(self, path, samples, block_rows=3000):
        self._path, self._tmp, self._rows, self._held, self._n_held = path, path + ".part", int(block_rows), [], 0
        self.n_samples, self.row_bytes = len(samples), row_bytes_for(len(samples))
        self._f = open(self._tmp, "wb")
        names = "\n".join(samples).encode()
        head = _CL_MAGIC + np.array([self.n_samples, self.row_bytes], dtype="<u4").tobytes() + np.array([len(names)], dtype="<u8").tobytes() + names
        self._f.write(head + b"\0" * _pad8(len(head)))

    def write(self, cb):
        """One CallBlock over the cache's samples, any number of variants."""
        if len(cb) == 0:
            return
        if cb.present.shape[1] != self.row_bytes or cb.missing.shape != cb.present.shape:
            raise ValueError("call cache: planes of %d bytes a row, %d expected" % (cb.present.shape[1], self.row_bytes))
        names = [bytes(cb.blob[cb.off[i]:cb.off[i + 1]]) for i in range(len(cb))]
        self._held.append((names, [m_.encode() for m_ in cb.messages], np.asarray(cb.skip), np.asarray(cb.present), np.asarray(cb.missing),
                           np.asarray(cb.n_present), np.asarray(cb.n_missing)))
        self._n_held += len(cb)
        while self._n_held >= self._rows:
            self._store(self._rows)

    def _store(self, nv):
        """The first nv held variants as one stored block."""
        parts, left, rest = [], nv, []
        for item in self._held:
            n = len(item[0])
            if left >= n:
                parts.append(item); left -= n
            elif left > 0:
                parts.append(tuple(x[:left] for x in item)); rest.append(tuple(x[left:] for x in item)); left = 0
            else:
                rest.append(item)
        self._held, self._n_held = rest, self._n_held - nv
        names = [x for it in parts for x in it[0]]
        msgs = [x for it in parts for x in it[1]]
        name_off, msg_off = np.zeros(nv + 1, dtype="<i8"), np.zeros(nv + 1, dtype="<i8")
        np.cumsum([len(x) for x in names], out=name_off[1:])
        np.cumsum([len(x) for x in msgs], out=msg_off[1:])
        f = self._f
        f.write(np.array([nv, int(name_off[-1]), int(msg_off[-1]), 0], dtype="<u8").tobytes())
        f.write(name_off.tobytes() + msg_off.tobytes())
        for k in (2, 5, 6):
            f.write(np.ascontiguousarray(np.concatenate([it[k] for it in parts]), dtype="<i4").tobytes())
        f.write(b"".join(names) + b"".join(msgs))
        f.write(b"\0" * _pad8(12 * nv + int(name_off[-1]) + int(msg_off[-1])))
        for k in (3, 4):
            for it in parts:
                f.write(np.ascontiguousarray(it[k], dtype=np.uint8).tobytes())

    def close(self):
        if self._f is not None:
            try:
                if self._n_held:
                    self._store(self._n_held)
                self._f.write(b"\0" * 32)
                self._f.flush()
                os.fsync(self._f.fileno())
            except BaseException:
                self.abort()
                raise
            self._f.close()
            self._f = None
            os.replace(self._tmp, self._path)

    def abort(self):
        """Drop what was written (the run did not finish): no cache."""
        if self._f is not None:
            try:
                self._f.close()
            except (IOError, OSError):
                pass
            self._f = None
            try:
                os.remove(self._tmp)
            except OSError:
                pass

    def __del__(self):
        try:
            self.abort()
        except Exception:
            pass


def open_call_cache(path):
    """A call cache mapped -> (stored sample names, stored row width, rows in all, blocks): blocks() yields every stored block as a CallBlock
    over the STORED samples whose planes are views of the mapping.  Every block header is walked here, before a plane is read: a file that is
    no call cache, or is truncated, raises IOError now."""
    import mmap
    cut = IOError("truncated call cache %s (delete it, or run without --load-calls)" % path)
    with open(path, "rb") as f:
        size = os.fstat(f.fileno()).st_size
        magic = f.read(8)
        if magic == _PK_MAGIC:
            raise IOError("%s is a packed k-mer cache, not a call cache (it is read by --load-packed)" % path)
        if magic != _CL_MAGIC:
            raise IOError("%s is not a call cache" % path)
        if size < 24:
            raise cut
        mm = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
    ns, rb = (int(x) for x in np.frombuffer(mm, dtype="<u4", count=2, offset=8))
    ln = int(np.frombuffer(mm, dtype="<u8", count=1, offset=16)[0])
    pos = 24 + ln + _pad8(24 + ln)
    if pos > size:
        raise cut
    stored = mm[24:24 + ln].decode().split("\n")
    if len(stored) != ns or rb != row_bytes_for(ns):
        raise IOError("call cache %s: its header does not agree with its sample list" % path)
    index = []
    while True:
        if pos + 32 > size:
            raise cut
        nv, nb, mb, _ = (int(x) for x in np.frombuffer(mm, dtype="<u8", count=4, offset=pos))
        if nv == 0:
            break
        meta = 16 * (nv + 1) + 12 * nv + nb + mb
        end = pos + 32 + meta + _pad8(meta) + 2 * nv * rb
        if end > size:
            raise cut
        index.append((pos + 32, nv, nb, mb))
        pos = end

    def blocks():
        for at, nv, nb, mb in index:
            name_off = np.frombuffer(mm, dtype="<i8", count=nv + 1, offset=at)
            msg_off = np.frombuffer(mm, dtype="<i8", count=nv + 1, offset=at + 8 * (nv + 1))
            ints = np.frombuffer(mm, dtype="<i4", count=3 * nv, offset=at + 16 * (nv + 1)).reshape(3, nv)
            text = at + 16 * (nv + 1) + 12 * nv
            blob = mm[text:text + nb]
            msgs = mm[text + nb:text + nb + mb]
            said = np.nonzero(np.diff(msg_off))[0]
            messages = [""] * nv
            for i in said:
                messages[i] = msgs[msg_off[i]:msg_off[i + 1]].decode()
            planes = text + nb + mb + _pad8(12 * nv + nb + mb)
            present = np.frombuffer(mm, dtype=np.uint8, count=nv * rb, offset=planes).reshape(nv, rb)
            missing = np.frombuffer(mm, dtype=np.uint8, count=nv * rb, offset=planes + nv * rb).reshape(nv, rb)
            yield CallBlock(blob, name_off, ints[0], present, missing, ints[1], ints[2], messages, said.astype(np.int64))
    return stored, rb, sum(x[1] for x in index), blocks


def join_call_blocks(group):
    """Whole CallBlocks behind one another as one."""
    if len(group) == 1:
        return group[0]
    blob = b"".join(bytes(g.blob) for g in group)
    base = np.cumsum([0] + [len(g.blob) for g in group[:-1]])
    rows = np.cumsum([0] + [len(g) for g in group[:-1]])
    off = np.concatenate([np.asarray(g.off[:-1]) + b for g, b in zip(group, base)] + [np.array([len(blob)], dtype=np.int64)])
    cat = lambda k: np.concatenate([getattr(g, k) for g in group])
    return CallBlock(blob, off, cat("skip"), cat("present"), cat("missing"), cat("n_present"), cat("n_missing"), [m_ for g in group for m_ in g.messages],
                     np.concatenate([np.asarray(g.msg_rows, dtype=np.int64) + r for g, r in zip(group, rows)]))


def call_cache_sample_map(stored, samples):
    """None where the cache's sample list is the run's own; else map[j] = the position of run sample j among the stored names.  ValueError, in
    one line, for a run sample the cache lacks, a sample listed twice on either side, or -- SEERHIP_ROUTE cache_select=0 -- any other list."""
    if stored == samples:
        return None
    if _route.route("cache_select") == "0":
        raise ValueError("call cache was written for a different sample list / order (%d vs %d samples)" % (len(stored), len(samples)))
    where = {}
    for i, s in enumerate(stored):
        if s in where:
            raise ValueError("the call cache lists sample %s twice: it is served to its own sample list only" % s)
        where[s] = i
    seen = set()
    for s in samples:
        if s not in where:
            raise ValueError("the call cache does not hold sample %s of the run" % s)
        if s in seen:
            raise ValueError("sample %s is listed twice in the run: a call cache is selected for distinct samples" % s)
        seen.add(s)
    return np.array([where[s] for s in samples], dtype=np.int32)


class SelectCallBlock(CallBlock):
    """A stored block over the cache's samples on its way to Job.submit_calls_select: n_present / n_missing are those of the stored samples until the
    device has selected it; the consumer says what say_call_block says once the block's own counts are back (Job.calls_counts)."""
    __slots__ = ("selector",)


def iter_call_cache_blocks(p, blocks, job_block, mode, selector=None, n_src=0, sample_map=None, max_missing=0.05, min_af=0.01, max_af=0.99, want_patterns=True):
    """The stream of a run from a call cache; blocks: the stored blocks' iterator open_call_cache returns.  Stored blocks are joined, whole, into groups
    of at most job_block variants (a stored block that is larger goes alone).
    mode "job": CallBlocks for Job.submit_calls, restricted to the run's samples where sample_map is given -- by selector.select_calls, or with
    selector None by the host restatement -- with their stderr lines said here; "fused": SelectCallBlocks over the stored samples for
    Job.submit_calls_select; "packed": the PackedBlocks of the Python block loop (_vcf_packed_block, which says the lines itself; want_patterns as there)."""
    from . import engine as _engine
    samples = [str(x) for x in p.index]
    order = sorted(range(len(samples)), key=lambda i: samples[i])

    def groups():
        acc, rows = [], 0
        for cb in blocks():
            if acc and rows + len(cb) > job_block:
                yield join_call_blocks(acc)
                acc, rows = [], 0
            acc.append(cb); rows += len(cb)
        if acc:
            yield join_call_blocks(acc)
    for cb in groups():
        if mode == "fused":
            cb = _job_call_block(cb)
            out = SelectCallBlock(cb.blob, cb.off, cb.skip, cb.present, cb.missing, cb.n_present, cb.n_missing, cb.messages, cb.msg_rows)
            out.selector = selector
            yield out
            continue
        if sample_map is not None:
            if selector is not None:
                sel = selector.select_calls(cb.present, cb.missing)
            else:
                sel = _engine.select_calls_host(cb.present, cb.missing, n_src, sample_map)
            cb = CallBlock(cb.blob, cb.off, cb.skip, sel[0], sel[1], sel[2], sel[3], cb.messages, cb.msg_rows)
        if mode == "packed":
            yield _vcf_packed_block(len(samples), samples, order, cb.names, cb.skip, cb.present, cb.missing, cb.n_present, cb.n_missing, min_af, max_af,
                                    max_missing, want_patterns, cb.messages)
        else:
            say_call_block(cb)
            yield _job_call_block(cb)


class _DmaWindows(object):
    """Windows of the packed-cache mapping registered with the HIP runtime (sh_host_register) so that a block's rows go from the page cache
    to the device by DMA, with no CPU copy (4 ns of CPU per 632-byte row against 21 for the copy into pinned staging:
    profiles/r05/host_feed_probe.txt).  Registering is cheap (1.2 ms per 160 MB, also with the device busy) but UNREGISTERING waits for the
    device to drain (28 ms per call under load, tools/gpu_probe_register.py): so a window spans several stored blocks (up to WINDOW bytes,
    cut at block boundaries: windows never share a page), is unregistered once all its blocks have been collected, and by a JANITOR thread of
    its own -- never by the thread that feeds the device, and since the lanes (a fixed-effects device is never idle between blocks: the
    reader thread, which did it until then, stood 0.33 of 1.2 s in hipHostUnregister) not by the reader either."""
    WINDOW = 1 << 30
    # hipHostUnregister waits for the device to drain AND holds new work back while it does: every call is a hole in the device's timeline
    # (16 windows of a 24 M-row fixed-effects job: 155 of 820 ms idle).  So finished windows stay registered (their pages pinned) until the
    # stream ends, or until more than KEEP bytes of them have piled up -- a quarter of the machine's memory, at most 64 GB per stream.
    # KEEP is the PROCESS's budget: a `--gpus G` job runs G streams, each with its own windows, and G x a quarter of the memory would be
    # twice the machine at G = 8: a stream's share is KEEP / (streams alive).
    try:
        KEEP = min(64 << 30, os.sysconf("SC_PHYS_PAGES") * os.sysconf("SC_PAGE_SIZE") // 4)
    except (ValueError, OSError, AttributeError):
        KEEP = 8 << 30
    PAGE = 4096                        # sh_host_register rounds a window out to whole pages
    _live = 0                          # streams with windows, process-wide
    _live_lock = None

    def _keep(self):
        return self.KEEP // max(1, _DmaWindows._live)

    def __init__(self, device):
        import threading
        from . import _abi
        if _DmaWindows._live_lock is None:
            _DmaWindows._live_lock = threading.Lock()
        with _DmaWindows._live_lock:
            _DmaWindows._live += 1
        self._counted = True
        self._lib = _abi.load()
        self._device = int(device)
        self._lock = threading.Lock()
        self._win_of = {}              # stored block -> window
        self._done = []                # windows whose blocks have all been collected, to unregister
        self._reader_done = False
        self.ok = True
        self._wake = threading.Condition(self._lock)
        self._janitor = None
        self._stop = False

    def plan(self, base_addr, extents, lo_blk, hi_blk):
        # Windows are registered rounded out to whole pages and must not overlap (registering a page twice fails): where less than a page
        # of metadata lies between two stored blocks (small blocks), the block that starts on the previous window's last page belongs to no
        # window -- its rows are staged -- and the next window starts at the first block on a page of its own.
        j, prev_end = lo_blk, 0
        while j < hi_blk:
            if ((base_addr + extents[j][0]) & ~(self.PAGE - 1)) < prev_end:
                j += 1
                continue
            k, lo = j, base_addr + extents[j][0]
            hi = lo + extents[j][1]
            while k + 1 < hi_blk and base_addr + extents[k + 1][0] + extents[k + 1][1] - lo <= self.WINDOW:
                k += 1
                hi = base_addr + extents[k][0] + extents[k][1]
            w = {"lo": lo, "n": hi - lo, "blocks": k - j + 1, "taken": 0, "released": 0, "state": 0}     # state 0 new, 1 registered, -1 refused
            for b in range(j, k + 1):
                self._win_of[b] = w
            prev_end = (hi + self.PAGE - 1) & ~(self.PAGE - 1)
            j = k + 1

    def _unregister_done(self):
        with self._lock:
            todo, self._done = self._done, []
        for w in todo:
            self._lib.sh_host_unregister(w["lo"])

    def _janitor_loop(self):
        while True:
            with self._wake:
                while not self._due() and not self._stop:
                    self._wake.wait()
                if not self._done and self._stop:
                    return
                todo = []
                if self._reader_done or self._stop:
                    todo, self._done = self._done, []
                else:
                    while self._done and sum(w["n"] for w in self._done) > self._keep():
                        todo.append(self._done.pop(0))
            for w in todo:
                self._lib.sh_host_unregister(w["lo"])

    def _due(self):
        """(lock held) is there a window to unregister NOW: the stream has ended, or too many finished windows are still pinned"""
        return bool(self._done) and (self._reader_done or sum(w["n"] for w in self._done) > self._keep())

    def _kick(self):
        """(lock held) a window is ready to be unregistered: wake the janitor, starting it at the first need"""
        if self._janitor is None:
            import threading
            self._janitor = threading.Thread(target=self._janitor_loop, daemon=True)
            self._janitor.start()
        self._wake.notify()

    def take(self, j):
        """(dma, release) for stored block j, called on the reader thread just before the block is handed on."""
        w = self._win_of.get(j)
        if w is None or not self.ok:
            return False, None
        if w["state"] == 0:
            if self._lib.sh_host_register(w["lo"], w["n"], self._device) != 0:
                w["state"] = -1
                self.ok = False        # (a file system whose pages cannot be pinned, or the pinning limit: the rows are staged through pinned memory from here on)
                sys.stderr.write("pyseer_amd: the packed-cache mapping cannot be registered for DMA (%s): this stream's rows are staged through pinned "
                                 "memory from here on (slower on the host, same results)\n" % self._lib.sh_last_error().decode())
                return False, None
            w["state"] = 1
        if w["state"] != 1:
            return False, None
        w["taken"] += 1

        def release():
            with self._lock:
                w["released"] += 1
                last = w["released"] == w["blocks"] or (self._reader_done and w["released"] == w["taken"])
                if last:
                    self._done.append(w)
                    self._kick()
        return True, release

    def reader_done(self):
        if self._counted:                                              # (this stream pins nothing new from here on: its share goes back)
            self._counted = False
            with _DmaWindows._live_lock:
                _DmaWindows._live -= 1
        with self._lock:
            self._reader_done = True
            for w in {id(x): x for x in self._win_of.values()}.values():
                if w["state"] == 1 and w["released"] == w["taken"] and w not in self._done and w["released"] < w["blocks"]:
                    self._done.append(w)
            if self._done:
                self._kick()


def _cache_sample_map(stored, samples, select):
    """The packed cache's stored sample names against the run's: None where they are the run's own list, else -- with `select` given and
    SEERHIP_ROUTE cache_select not 0 -- the int32 table map[j] = position of run sample j among the stored names, for a cache whose names are
    distinct and hold every run sample once.  Raises the ValueError every other cache has always met."""
    if stored == samples:
        return None
    if select is not None and _route.route("cache_select") != "0" and len(set(stored)) == len(stored) and len(set(samples)) == len(samples):
        where = {s: i for i, s in enumerate(stored)}
        if all(s in where for s in samples):
            return np.array([where[s] for s in samples], dtype=np.int32)
    raise ValueError("packed cache was written for a different sample list / order (%d vs %d samples)" % (len(stored), len(samples)))


def _open_selector(select, n_src, sample_map):
    """rows -> (rows, counts) over the run's samples: on the device of the Engine `select` (k_rows_select), or by the host restatement
    (select == "host", or SEERHIP_ROUTE cache_select=host); and what closes it."""
    from . import engine as _engine
    if select == "host" or _route.route("cache_select") == "host":
        return (lambda bits: _engine.select_rows_host(bits, n_src, sample_map)), (lambda: None)
    sel = _engine.RowSelector(select, n_src, sample_map)
    return sel.select, sel.close


def check_packed_cache(p, path, select=None):
    """The header checks of iter_packed_blocks_cached without reading a block (the library's own block loop, sh_job_run_packed, walks the file
    itself): magic, sample list and order, row width.  Raises what the iterator raises.  select (an Engine, "host", or anything but None):
    a cache over a superset or another order of the samples is accepted as the iterator accepts it; returns its sample map, else None."""
    samples = [str(x) for x in p.index]
    with open(path, "rb") as f:
        head = f.read(24)
        if head[:8] == _CL_MAGIC:
            raise IOError("%s is a call cache, not a packed k-mer cache (it is read by --load-calls)" % path)
        if len(head) < 24 or head[:8] != _PK_MAGIC:
            raise IOError("%s is not a packed k-mer cache" % path)
        ns, rb = np.frombuffer(head, dtype="<u4", count=2, offset=8)
        (ln,) = np.frombuffer(head, dtype="<u8", count=1, offset=16)
        names = f.read(int(ln))
        if len(names) < int(ln):
            raise IOError("truncated packed cache %s (delete it, or run without --load-packed)" % path)
    stored = names.decode().split("\n")
    sample_map = _cache_sample_map(stored, samples, select)
    if int(rb) != row_bytes_for(len(stored)):
        raise IOError("packed cache row width mismatch")
    return sample_map


def _map_packed_cache(path):
    """The cache memory-mapped and its header read -> (mapping, its size, stored sample names, stored row width, offset of the first block).
    A block's bit rows are a VIEW into the mapping (round 3: f.read() of a 170 MB block was a 40 ms copy per block, more than the GPU needs
    to test it): the engine's host-to-device copy reads the page cache directly."""
    import mmap
    with open(path, "rb") as f:
        size = os.fstat(f.fileno()).st_size
        if size < 24:
            raise IOError("%s is not a packed k-mer cache" % path)
        mm = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
    try:
        mm.madvise(mmap.MADV_SEQUENTIAL)
    except (AttributeError, OSError):
        pass
    if mm[:8] == _CL_MAGIC:
        raise IOError("%s is a call cache, not a packed k-mer cache (it is read by --load-calls)" % path)
    if mm[:8] != _PK_MAGIC:
        raise IOError("%s is not a packed k-mer cache" % path)
    ns, rb = np.frombuffer(mm, dtype="<u4", count=2, offset=8)
    (ln,) = np.frombuffer(mm, dtype="<u8", count=1, offset=16)
    pos = 24 + int(ln)
    if pos > size:
        raise IOError("truncated packed cache %s (delete it, or run without --load-packed)" % path)
    return mm, size, mm[24:pos].decode().split("\n"), int(rb), pos


def _packed_block_extents(mm, pos, size, rb, path):
    """The index pass over a mapped cache from its first block at `pos`: the 16-byte header of every stored block, up to the terminator (a few
    hundred bytes of the mapping are touched) -> (rows of every stored block, (offset, bytes) of its bit rows, (offset, name bytes) of what
    precedes them: name offsets, counts, names).  A cache that ends before its terminator raises the IOError every truncated cache meets."""
    nvs, extents, metas = [], [], []
    while True:
        if pos + 16 > size:
            raise IOError("truncated packed cache %s (delete it, or run without --load-packed)" % path)
        nv, nb = (int(x) for x in np.frombuffer(mm, dtype="<u8", count=2, offset=pos))
        pos += 16
        if nv == 0:
            return nvs, extents, metas
        metas.append((pos, nb))
        pos += 8 * (nv + 1) + 4 * nv + nb
        if pos + nv * rb > size:
            raise IOError("truncated packed cache %s (delete it, or run without --load-packed)" % path)
        extents.append((pos, nv * rb))
        nvs.append(nv)
        pos += nv * rb


def open_packed_cache_rows(path):
    """A packed cache's stored rows as they lie in the file, for a consumer that restricts them to its samples itself (similarity
    --load-packed: RowSelector.sim_accumulate) -> (stored sample names, stored row width, total rows, rows): rows() yields per stored block
    its (nv, row width) uint8 rows, a view of the mapping, and (row, name) of its lines that no stored sample carries.  Every block header is
    walked here, before a row is read: a cache that is not one, or is truncated, raises IOError now."""
    mm, size, stored, rb, pos = _map_packed_cache(path)
    if rb != row_bytes_for(len(stored)):
        raise IOError("packed cache row width mismatch")
    nvs, extents, metas = _packed_block_extents(mm, pos, size, rb, path)

    def rows():
        for nv, (at, nbytes), (meta, nb) in zip(nvs, extents, metas):
            counts = np.frombuffer(mm, dtype="<i4", count=nv, offset=meta + 8 * (nv + 1))
            empty = []
            if not counts.all():
                off = np.frombuffer(mm, dtype="<i8", count=nv + 1, offset=meta)
                names = meta + 8 * (nv + 1) + 4 * nv
                empty = [(int(i), mm[names + int(off[i]):names + int(off[i + 1])].decode()) for i in np.nonzero(counts == 0)[0]]
            yield np.frombuffer(mm, dtype=np.uint8, count=nbytes, offset=at).reshape(nv, rb), empty
    return stored, rb, sum(nvs), rows


def iter_packed_blocks_cached(p, path, min_af, max_af, block_size, want_patterns=False, want_samples=False, part=None, raw=False, device=None, ahead=2,
                              say_empty=True, select=None):
    """PackedBlock stream from a packed cache written by --save-packed; the samples (and their order) must be the run's own.
    select: an Engine over the run's samples, or "host" -- a cache whose stored names are distinct and hold every run sample is accepted too:
    every stored block's rows are restricted to the run's samples and brought into their order (engine.RowSelector on that engine's device;
    "host": engine.select_rows_host) and its counts taken anew, on the reader thread, before blocks are merged; such rows are never handed
    on as DMA windows.  A cache with the run's own list takes the path it always took.
    Stored blocks are re-cut to about `block_size` variants (stored blocks are never split, only merged).
    part = (i, n): only range i of n contiguous ranges of the cache's rows (the multi-GPU job: one range per device,
    pyseer_amd/__main__.py).  Ranges are made of whole blocks of the single stream, so the n parts yield exactly its blocks; they are
    as equal as block_size allows (a cache of B blocks over n devices: ceil(B/n) against floor(B/n) blocks).
    raw: RawBlock objects for the job stream; with `device` given, a block that is one stored block (no merge) is handed on as a window of the
    mapping registered for DMA (sh_host_register: the rows go from the page cache to the device with no CPU copy).
    ahead: blocks the reader thread runs ahead of the consumer (the job stream of a fixed-effects model holds 2 + lanes blocks in flight)."""
    samples = [str(x) for x in p.index]
    order = sorted(range(len(samples)), key=lambda i: samples[i])
    n = len(samples)

    def raw_blocks():
        mm, size, stored, rb, pos = _map_packed_cache(path)
        sample_map = _cache_sample_map(stored, samples, select)
        if rb != row_bytes_for(len(stored)):
            raise IOError("packed cache row width mismatch")
        select_rows, select_close = (None, None) if sample_map is None else _open_selector(select, len(stored), sample_map)
        use_dma = want_dma and sample_map is None
        windows = _DmaWindows(device) if use_dma else None
        windows_box.append(windows)

        def need(nbytes):
            nonlocal pos
            if pos + nbytes > size:
                raise IOError("truncated packed cache %s (delete it, or run without --load-packed)" % path)
            at = pos
            pos += nbytes
            return at
        lo_blk, hi_blk = 0, None
        extents = None                                     # (offset, bytes) of every stored block's bit rows, when somebody needs them up front
        if part is not None or use_dma:
            # index pass: the 16-byte header of every stored block (a few hundred bytes of the mapping are touched).  The single stream merges
            # stored blocks until it holds block_size rows (merged() below); a part owns whole such groups -- the groups whose first row falls
            # into its share of the rows -- so every part hands the engine exactly the blocks the single stream would, and output that depends
            # on where blocks end (fit_lmm's filtered-first order, its stale-k lineage: pyseer/lmm.py:160-217) does not change
            nvs, extents, _ = _packed_block_extents(mm, pos, size, rb, path)
        if part is not None:
            total = sum(nvs)
            i_, n_ = part
            owner, first_row, rows, row0 = [], 0, 0, 0
            for j, nv in enumerate(nvs):
                if rows == 0:
                    first_row = row0
                owner.append(min(n_ - 1, (first_row * n_) // max(total, 1)))
                rows += nv; row0 += nv
                if rows >= block_size:
                    rows = 0
            mine = [j for j, o in enumerate(owner) if o == i_]
            lo_blk, hi_blk = (mine[0], mine[-1] + 1) if mine else (0, 0)
        if use_dma:
            windows.plan(np.frombuffer(mm, dtype=np.uint8, count=1).ctypes.data, extents, lo_blk, len(extents) if hi_blk is None else hi_blk)
        j = -1
        try:
            while True:
                at = need(16)
                nv, nb = (int(x) for x in np.frombuffer(mm, dtype="<u8", count=2, offset=at))
                if nv == 0:
                    return
                j += 1
                if hi_blk is not None and not (lo_blk <= j < hi_blk):                      # a stored block of another part: skipped unread
                    if j >= hi_blk:
                        return
                    need(8 * (nv + 1) + 4 * nv + nb + nv * rb)
                    continue
                off = np.frombuffer(mm, dtype="<i8", count=nv + 1, offset=need(8 * (nv + 1)))
                counts = np.frombuffer(mm, dtype="<i4", count=nv, offset=need(4 * nv))
                at = need(nb)
                blob = np.frombuffer(mm, dtype=np.uint8, count=nb, offset=at) if raw else mm[at:at + nb]  # (raw: a view, the names are only read for printed rows)
                bits = np.frombuffer(mm, dtype=np.uint8, count=nv * rb, offset=need(nv * rb)).reshape(nv, rb)
                if select_rows is not None:                                                # (the stored counts are those of the cache's samples)
                    bits, counts = select_rows(bits)
                yield blob, off, counts, bits, j
        finally:
            if select_close is not None:
                select_close()

    def merged():
        acc, rows = [], 0
        for blk in raw_blocks():
            acc.append(blk); rows += blk[2].shape[0]
            if rows >= block_size:
                yield acc
                acc, rows = [], 0
        if acc:
            yield acc

    want_dma = raw and device is not None and _route.route("dma", "1") != "0"
    windows_box = []                     # the stream's DMA windows, or None: known once the header has been read (a selected cache has none)

    def finished():                      # merging and a block's host preparation (6 ms per 262 144 rows) on the reader's thread, ahead of the engine
        windows = None
        try:
            for group in merged():
                windows = windows_box[0]
                if raw and len(group) == 1:
                    blob, off, counts, bits, j = group[0]
                    dma, release = windows.take(j) if windows is not None else (False, None)
                    yield _raw_block(blob, off, counts, bits, dma, release, say_empty=say_empty)
                    continue
                if len(group) == 1:
                    blob, off, counts, bits, _ = group[0]
                else:
                    blob = b"".join(bytes(g[0]) for g in group)
                    base = np.cumsum([0] + [len(g[0]) for g in group[:-1]])
                    off = np.concatenate([g[1][:-1] + b for g, b in zip(group, base)] + [np.array([len(blob)], dtype=np.int64)])
                    counts = np.concatenate([g[2] for g in group])
                    bits = np.concatenate([g[3] for g in group], axis=0)
                if raw:
                    yield _raw_block(blob, off, counts, bits, say_empty=say_empty)
                    continue
                yield _block_from_raw(n, samples, order, None, blob, off, bits, counts, min_af, max_af, want_patterns, want_samples)
        finally:
            if windows is not None:
                windows.reader_done()

    for blk in prefetched(finished(), depth=max(2, int(ahead))):
        yield blk


# ---------------------------------------------------------------------------------------------------------------
# the command line's k-mer stream: which of text, --load-packed and --packed-cache a run reads, shared by the per-variant run and --wg enet
# ---------------------------------------------------------------------------------------------------------------
def check_kmers_gzipped(paths):
    """The reference's gzip.open raises on plain text (input.py:271-276); the native reader would read it, so the command line asks."""
    for vf in paths:
        with open(vf, "rb") as fh:
            if fh.read(2) != b"\x1f\x8b":
                sys.stderr.write("Not a gzipped file (%s): use --uncompressed for plain-text k-mers\n" % vf)
                sys.exit(1)


def plan_packed_cache(options, p, var_file, read_first_block=True):
    """--packed-cache, the automatic form of --save-packed / --load-packed: one file next to the input, tied to it by size + mtime (a sidecar
    stamp), and to the run by the sample list the cache itself stores.  Sets options.load_packed (a fresh cache is read) or
    options.save_packed (one is written); returns the stamp (sidecar path, text) for the PackedCacheWriter, or None.
    read_first_block: check the cache by reading its first block, as the per-variant run always has (which says "No observations of ..." for
    that block's empty lines once more); False checks the header alone (check_packed_cache: the same errors, nothing on stderr)."""
    cache_stamp = None
    side = var_file + ".seerpack"
    st = os.stat(var_file)
    stamp = "%d %d" % (st.st_size, int(st.st_mtime))
    fresh = False
    try:
        fresh = os.path.exists(side) and open(side + ".stamp").read().strip() == stamp
    except (IOError, OSError):
        fresh = False
    if fresh and not packed_cache_complete(side):
        sys.stderr.write("Packed cache %s is incomplete (an interrupted run); parsing %s again\n" % (side, var_file))
        fresh = False
    if fresh:
        try:
            if read_first_block:
                next(iter(iter_packed_blocks_cached(p, side, options.min_af, options.max_af, 1)), None)    # header + sample list check
            else:
                check_packed_cache(p, side)
            options.load_packed = side
        except ValueError:
            sys.stderr.write("Packed cache %s was written for other samples; parsing %s again\n" % (side, var_file))
            fresh = False
        except IOError as ex:
            sys.stderr.write("Packed cache %s cannot be used (%s); parsing %s again\n" % (side, ex, var_file))
            fresh = False
    if not fresh:
        # the cache is written to a temporary name and renamed when the run has read the whole input; the stamp follows the rename
        # (PackedCacheWriter.close), so an interrupted run leaves neither
        if os.access(os.path.dirname(os.path.abspath(side)) or ".", os.W_OK):
            options.save_packed = side
            cache_stamp = (side + ".stamp", stamp)
        else:
            sys.stderr.write("Cannot write a packed cache next to %s; continuing without\n" % var_file)
    return cache_stamp


def announce_cache_select(p, path, select):
    """--load-packed of the command line: the header checks (check_packed_cache), and for a cache over a superset or another order of the
    run's samples the one line that says so.  Returns True for such a cache."""
    sample_map = check_packed_cache(p, path, select=select)
    if sample_map is None:
        return False
    with open(path, "rb") as f:
        (stored,) = np.frombuffer(f.read(12), dtype="<u4", count=1, offset=8)
    where = "host" if (select == "host" or _route.route("cache_select") == "host") else "device"
    sys.stderr.write("pyseer_amd: packed cache holds %d samples; the run's %d are selected on the %s\n" % (int(stored), len(p), where))
    return True


def open_kmer_block_stream(options, p, kmer_files, block_size, select=None):
    """The RawBlock stream of a run that takes every parsed line as it is (--wg enet: the device applies its own rule), from what the
    command line names: --load-packed, --packed-cache, one or several --kmers files.  Returns (blocks, PackedCacheWriter or None): the
    caller closes the writer once the stream has ended.  The cache is read through the page cache (device=None: no registered windows).
    select: the run's Engine -- a --load-packed cache over a superset or another order of the samples is served through it."""
    cache_out = cache_stamp = None
    if not options.uncompressed and not options.load_packed:
        check_kmers_gzipped(kmer_files)
    if options.packed_cache and not options.load_packed and not options.save_packed:
        cache_stamp = plan_packed_cache(options, p, kmer_files[0], read_first_block=False)
    if options.load_packed:
        if select is not None:
            announce_cache_select(p, options.load_packed, select)
        return iter_packed_blocks_cached(p, options.load_packed, options.min_af, options.max_af, block_size, raw=True, device=None, select=select), None
    if len(kmer_files) > 1:
        return iter_packed_blocks_native_multi(p, kmer_files, options.min_af, options.max_af, block_size, raw=True), None
    if options.save_packed:
        cache_out = PackedCacheWriter(options.save_packed, [str(x) for x in p.index], stamp=cache_stamp)
    return iter_packed_blocks_native(p, kmer_files[0], options.min_af, options.max_af, block_size, save_to=cache_out, raw=True), cache_out
