"""VCF and burden input on the device: the native reader (sh_vcf_*: csrc/vcf_reader.cpp on the host, k_vcf_gt_pack and k_burden_fold in
csrc/vcf_kernels.hip) against the Python text reader, and the command line against the reference's recorded runs
(tests/golden/vcf/lmm50_expected.*: the rows of the reference's tests/baseline/23.log that belong to records of variants50.vcf.gz;
burden_expected.tsv: the projection-independent columns of its 13.log / 37.log).  tests/golden/make_vcf_fixtures.py wrote the fixtures."""
import collections
import contextlib
import io
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
pytestmark = pytest.mark.gpu

from _vcf_text import generated_vcf, write_bgzf  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "golden", "cli")
VCF = os.path.join(ROOT, "tests", "golden", "vcf")
TIMEOUT = 600


def _num_close(a, b, sign_free=False):
    """tests/test_cli_gpu.py's rule for two '%.2E' strings: equal, within the Firth noise floor around zero, or one unit of the last printed digit apart."""
    if a == b:
        return True
    if a == "" or b == "":
        return False
    x, y = float(a), float(b)
    if sign_free:
        x, y = abs(x), abs(y)
    if abs(x - y) <= 1e-6:
        return True
    if x == 0.0 or y == 0.0 or (x > 0) != (y > 0):
        return False
    import math
    ex = math.floor(math.log10(max(abs(x), abs(y))))
    mx, my = round(abs(x) / 10.0 ** (ex - 2)), round(abs(y) / 10.0 ** (ex - 2))
    return abs(mx - my) <= 1


def _pheno():
    p = pd.read_csv(os.path.join(CLI, "subset.pheno"), index_col=0, sep="\t")["binary"]
    p.index = p.index.astype(str)
    return p


def _cli(args, module="pyseer_amd", cwd=CLI):
    env = dict(os.environ); env["PYTHONPATH"] = ROOT
    r = subprocess.run([sys.executable, "-m", module] + args, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=TIMEOUT)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return r.stdout.decode(), r.stderr.decode()


# ---- 5. native = Python, record by record ---------------------------------------------------------------------------------------------------
def _python_records(path, samples):
    """names, skip reasons, present / missing rows over `samples` and their counts, from the Python text reader."""
    from pyseer_amd.input import VcfFile
    from pyseer_amd.packing import pack_variants
    f = VcfFile(path)
    names, skip, pres, miss = [], [], [], []
    keep = set(samples)
    with contextlib.redirect_stderr(io.StringIO()):
        for rec in f:
            d = {}
            f.apply(rec, d)
            names.append(rec.name); skip.append(rec.skip)
            pres.append([1 if (s in keep and d.get(s) == 1) else 0 for s in samples])
            miss.append([1 if (s in d and d[s] != 1) else 0 for s in samples])
    pres, miss = np.array(pres, dtype=np.uint8).reshape(len(names), len(samples)), np.array(miss, dtype=np.uint8).reshape(len(names), len(samples))
    return names, np.array(skip), pack_variants(pres), pack_variants(miss), pres.sum(axis=1), miss.sum(axis=1)


def _native_records(path, samples, engine, block_size):
    from pyseer_amd.input import NativeVcfReader
    r = NativeVcfReader(path, samples, engine, block_size)
    names, parts = [], collections.defaultdict(list)
    for rb in r.raw_blocks():
        assert 1 <= len(rb["skip"]) <= block_size
        names += [rb["blob"][rb["off"][i]:rb["off"][i + 1]].decode() for i in range(len(rb["skip"]))]
        for key in ("skip", "present", "missing", "n_present", "n_missing"):
            parts[key].append(rb[key].copy())
    info = r.info()
    r.close()
    return (names,) + tuple(np.concatenate(parts[k]) for k in ("skip", "present", "missing", "n_present", "n_missing")) + (info,)


def _assert_native_equals_python(path, samples, engine, block_sizes=(1, 7, 3000)):
    want = _python_records(path, samples)
    for bs in block_sizes:
        got = _native_records(path, samples, engine, bs)
        assert got[0] == want[0], "names, block size %d" % bs
        for j, what in ((1, "skip reasons"), (2, "present rows"), (3, "missing rows"), (4, "present counts"), (5, "missing counts")):
            assert np.array_equal(got[j], want[j]), "%s, block size %d: first difference at record %d" % (
                what, bs, int(np.nonzero(np.asarray(got[j] != want[j]).reshape(len(want[0]), -1).any(axis=1))[0][0]))
    return got[6]


@pytest.mark.parametrize("name", ["variants50.vcf.gz", "variants_missing.vcf.gz", "variants_no_gt.vcf.gz", "variants_head.vcf.gz"])
def test_native_reader_equals_python_reader_on_fixtures(name):
    from pyseer_amd.engine import Engine
    samples = list(_pheno().index)
    e = Engine(len(samples))
    try:
        _assert_native_equals_python(os.path.join(VCF, name), samples, e)
        if name == "variants_head.vcf.gz":                                     # and over all of the file's own samples, in its own order
            from pyseer_amd.input import VcfFile
            every = VcfFile(os.path.join(VCF, name)).samples
            e2 = Engine(len(every))
            try:
                _assert_native_equals_python(os.path.join(VCF, name), every, e2)
            finally:
                e2.close()
    finally:
        e.close()


@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    """N = 5000 phenotyped samples among 5200 shuffled columns, 2000 records: 1-byte and 20-byte sample fields, GT second in FORMAT, haploid and
    diploid calls, ~3 % missing, multi-allelic and filtered records, records without GT; BGZF, gzip and (cut short, without its last newline) plain."""
    import gzip
    d = tmp_path_factory.mktemp("vcfgen")
    text, pheno, cols = generated_vcf(n_pheno=5000, n_cols=5200, n_records=2000, seed=7, missing=0.03)
    paths = {"bgzf": str(d / "gen.vcf.gz"), "gzip": str(d / "gen_small.vcf.gz"), "plain": str(d / "gen_small.vcf")}
    write_bgzf(paths["bgzf"], text, level=1)
    cut = text[:text.index(b"\n", len(text) // 20)]                            # the first twentieth, ending without a newline
    with gzip.open(paths["gzip"], "wb", compresslevel=1) as f:
        f.write(cut)
    open(paths["plain"], "wb").write(cut)
    regions = d / "regions.txt"
    rng = np.random.RandomState(5)
    lines = []
    for g in range(300):
        regs = []
        for _ in range(1 + (g % 3 == 0) + (g % 7 == 0)):
            contig = "chr1" if rng.randint(3) else "chr2"
            start = int(rng.randint(1, 27000 if contig == "chr1" else 14000))
            regs.append("%s:%d-%d" % (contig, start, start + int(rng.randint(0, 400))))
        lines.append("gene%03d %s" % (g, ",".join(regs)))
    lines[17] = "gene017 chr1:77"                                              # does not parse
    lines[18] = "gene018 chr9:1-100000"                                        # a contig the file does not have
    regions.write_text("\n".join(lines) + "\n")
    return {"paths": paths, "pheno": pheno, "regions": str(regions), "text_bytes": len(text)}


def test_native_reader_equals_python_reader_on_generated_file(generated):
    from pyseer_amd.engine import Engine
    e = Engine(5000)
    try:
        info = _assert_native_equals_python(generated["paths"]["bgzf"], generated["pheno"], e)
        assert info == {"container": "bgzf", "columns": 5200, "contigs": 2}
        assert _assert_native_equals_python(generated["paths"]["gzip"], generated["pheno"], e, (7, 3000))["container"] == "gzip"
        assert _assert_native_equals_python(generated["paths"]["plain"], generated["pheno"], e, (7, 3000))["container"] == "plain"
    finally:
        e.close()


# ---- 6. k_burden_fold -----------------------------------------------------------------------------------------------------------------------
def _blocks_equal(a, b):
    assert len(a) == len(b), (len(a), len(b))
    for x, y in zip(a, b):
        assert list(x.names) == list(y.names)
        assert list(x.status) == list(y.status)
        assert np.array_equal(np.asarray(x.afs, float), np.asarray(y.afs, float), equal_nan=True)
        assert [list(k) for k in x.kstrains] == [list(k) for k in y.kstrains] and [list(k) for k in x.nkstrains] == [list(k) for k in y.nkstrains]
        assert list(x.patterns) == list(y.patterns)
        assert np.array_equal(x.bits, y.bits) and list(x.row_of) == list(y.row_of)
        for k1, k2 in zip(x.ks, y.ks):
            assert (k1 is None) == (k2 is None) and (k1 is None or (k1.dtype == k2.dtype and np.array_equal(k1, k2, equal_nan=True)))


def _burden_both(path, regions_file, p, engine, block_size, max_missing=0.05):
    from pyseer_amd.input import iter_packed_blocks, iter_packed_blocks_vcf_native, load_burden, open_variant_file
    e1, e2 = io.StringIO(), io.StringIO()
    with contextlib.redirect_stderr(e1):
        regions = collections.deque()
        infile, order = open_variant_file("vcf", path, regions_file, regions)
        a = list(iter_packed_blocks(p, "vcf", infile, set(p.index), order, 0.01, 0.99, max_missing, False, block_size, burden=True, burden_regions=regions))
    with contextlib.redirect_stderr(e2):
        lst = []
        load_burden(regions_file, lst)
        b = list(iter_packed_blocks_vcf_native(p, path, engine, 0.01, 0.99, max_missing, block_size, burden_regions=lst))
    _blocks_equal(a, b)
    assert e1.getvalue() == e2.getvalue()
    return a


def test_burden_fold_equals_python_reader(generated):
    from pyseer_amd.engine import Engine
    p = _pheno()
    e = Engine(len(p))
    try:
        for regions in ("burden_regions.txt", "burden_regions_multiple.txt"):
            blocks = _burden_both(os.path.join(VCF, "variants50.vcf.gz"), os.path.join(VCF, regions), p, e, 2)
        assert [a for b in blocks for a in b.afs] == [0.08, 0.14, 0.22]
        _burden_both(os.path.join(VCF, "variants_missing.vcf.gz"), os.path.join(VCF, "burden_missing.txt"), p, e, 3000)
    finally:
        e.close()
    p5 = _pheno().head(5)
    e = Engine(5)
    try:
        blocks = _burden_both(os.path.join(VCF, "variants_missing.vcf.gz"), os.path.join(VCF, "burden_missing.txt"), p5, e, 3000)
        assert blocks[0].afs == [0.4] and blocks[0].bits.tolist()[0][0] == 3
    finally:
        e.close()
    pg = pd.Series(np.arange(5000) % 2, index=generated["pheno"])
    e = Engine(5000)
    try:
        for bs in (7, 3000):
            blocks = _burden_both(generated["paths"]["bgzf"], generated["regions"], pg, e, bs, max_missing=0.5)
        st = [s for b in blocks for s in b.status]
        assert len(st) == 300 and 2 in st and 0 in st and 1 in st              # rows with missing calls, clean rows, filtered ones
    finally:
        e.close()


# ---- 7. the command line against the reference's recorded LMM run ---------------------------------------------------------------------------
def test_cli_lmm_matches_the_reference_run():
    out, err = _cli(["--vcf", os.path.join(VCF, "variants50.vcf.gz"), "--phenotypes", "subset.pheno", "--similarity", "similarity50.tsv", "--lmm"])
    got = out.splitlines()
    want = open(os.path.join(VCF, "lmm50_expected.log")).read().splitlines()
    assert got[0] == want[0] and len(want) == 91
    for g, w in zip(got[1:], want[1:]):
        print(g, "|", w)
    assert [g.split("\t")[0] for g in got[1:]] == [w.split("\t")[0] for w in want[1:]]
    bad = []
    for g, w in zip(got[1:], want[1:]):
        gf, wf = g.split("\t"), w.split("\t")
        ok = len(gf) == len(wf) and set(gf[-1].split(",")) == set(wf[-1].split(",")) and all(_num_close(a, b) for a, b in zip(gf[1:-1], wf[1:-1]))
        if not ok:
            bad.append((g, w))
    assert not bad, bad
    exp = open(os.path.join(VCF, "lmm50_expected.err")).read().splitlines()
    lines = err.splitlines()
    for kind in ("Multiple alleles", "No observations"):
        assert [l for l in lines if l.startswith(kind)] == [l for l in exp if l.startswith(kind)], kind
    assert [l for l in lines if l.endswith("variants")] == [l for l in exp if l.endswith("variants")]
    assert [l for l in lines if l.endswith("variants")] == ["254 loaded variants", "164 pre-filtered variants", "90 tested variants", "90 printed variants"]


# ---- 8. burden through the command line ------------------------------------------------------------------------------------------------------
def test_cli_burden_matches_the_reference_run():
    out, err = _cli(["--vcf", os.path.join(VCF, "variants50.vcf.gz"), "--burden", os.path.join(VCF, "burden_regions_multiple.txt"),
                     "--phenotypes", "subset.pheno", "--no-distances"])
    got = [l.split("\t") for l in out.splitlines()]
    want = [l.split("\t") for l in open(os.path.join(VCF, "burden_expected.tsv")).read().splitlines()]
    assert got[0][:3] == want[0] and [g[0] for g in got[1:]] == ["CDS1", "CDS2", "CDS3"]
    for g, w in zip(got[1:], want[1:]):
        print(g, w)
        assert g[1] == w[1] and _num_close(g[2], w[2]), (g, w)
    assert [l for l in err.splitlines() if l.endswith("variants")] == ["3 loaded variants", "0 pre-filtered variants", "3 tested variants", "3 printed variants"]
    r = subprocess.run([sys.executable, "-m", "pyseer_amd", "--kmers", "kmers.gz", "--burden", os.path.join(VCF, "burden_regions.txt"), "--phenotypes",
                        "subset.pheno", "--no-distances"], cwd=CLI, env=dict(os.environ, PYTHONPATH=ROOT), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=TIMEOUT)
    assert r.returncode == 1 and r.stderr.decode().endswith("Burden test can only be performed with VCF input\n")


# ---- 9. the two readers through the command line: byte-identical -----------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["fixed", "lmm"])
@pytest.mark.parametrize("vcf", ["variants50.vcf.gz", "variants_missing.vcf.gz"])
def test_cli_native_and_python_readers_are_byte_identical(model, vcf, tmp_path):
    base = ["--vcf", os.path.join(VCF, vcf), "--phenotypes", "subset.pheno", "--print-samples", "--print-filtered", "--max-missing", "0.5"]
    base += ["--distances", "distances50.tsv"] if model == "fixed" else ["--similarity", "similarity50.tsv", "--lmm"]
    runs = []
    for extra in ([], ["--python-reader"]):
        pat = str(tmp_path / ("patterns%d.txt" % len(runs)))
        out, err = _cli(base + ["--output-patterns", pat] + extra)
        runs.append((out, err, open(pat, "rb").read()))
    assert runs[0][0] == runs[1][0]
    assert runs[0][1] == runs[1][1]
    assert runs[0][2] == runs[1][2] and len(runs[0][2]) > 0
    assert len(runs[0][0].splitlines()) > 1


def test_similarity_vcf_readers_agree_and_equal_numpy(tmp_path):
    samples = os.path.join(CLI, "samples50.txt")
    names = [l.rstrip() for l in open(samples)]
    path = os.path.join(VCF, "variants50.vcf.gz")
    a = _cli([samples, "--vcf", path], module="pyseer_amd.similarity")
    b = _cli([samples, "--vcf", path, "--python-reader"], module="pyseer_amd.similarity")
    assert a == b
    # G G^T from the Python reader's rows (pyseer/similarity.py:99-113: the AF- and missing-filtered variants)
    from pyseer_amd.input import open_variant_file, read_variant
    p = pd.Series(np.zeros(len(names)), index=names)
    infile, order = open_variant_file("vcf", path)
    cols = []
    with contextlib.redirect_stderr(io.StringIO()):
        while True:
            eof, k, name, ks, nks, af, missing = read_variant(infile, p, "vcf", False, None, False, set(p.index), order)
            if eof:
                break
            if k is not None and 0.01 <= af <= 0.99 and not missing > 0.05:
                cols.append(k)
    G = np.array(cols, dtype=float).T
    K = pd.read_csv(io.StringIO(a[0]), sep="\t", index_col=0)
    assert list(K.index) == names and G.shape[1] > 50 and np.array_equal(K.values, G.dot(G.T))


# ---- 10. missing calls: the VCF route and the Rtab route give the same rows -------------------------------------------------------------------
@pytest.mark.parametrize("model", ["fixed", "lmm"])
def test_missing_calls_take_the_rtab_path(model, tmp_path):
    """kmers120.Rtab (tests/golden/make_cli_golden.py: rows with one missing call, 2 % <= --max-missing, and rows with five, 10 % -> filtered) with
    every call re-expressed as a haploid GT; the two inputs must give the same output but for the variant names."""
    lines = open(os.path.join(CLI, "kmers120.Rtab")).read().splitlines()
    cols = lines[0].split("\t")[1:]
    vcf = tmp_path / "as_rtab.vcf"
    names = {}
    with open(str(vcf), "w") as f:
        f.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(cols) + "\n")
        for i, l in enumerate(lines[1:]):
            fields = l.split("\t")
            names["chrR_%d_A_C" % (i + 1)] = fields[0]
            f.write("\t".join(["chrR", str(i + 1), ".", "A", "C", ".", "PASS", ".", "GT:DP"] + [c + ":7" for c in fields[1:]]) + "\n")
    tail = ["--phenotypes", "subset.pheno", "--print-filtered"] + (["--distances", "distances50.tsv"] if model == "fixed" else ["--similarity", "similarity50.tsv", "--lmm"])
    want_out, want_err = _cli(["--pres", "kmers120.Rtab"] + tail)
    for extra in ([], ["--python-reader"]):
        out, err = _cli(["--vcf", str(vcf)] + tail + extra)
        renamed = "\n".join("\t".join([names.get(l.split("\t")[0], l.split("\t")[0])] + l.split("\t")[1:]) for l in out.splitlines()) + "\n"
        assert renamed == want_out
        for old, new in names.items():
            err = err.replace("of " + old + " in", "of " + new + " in")
        assert err == want_err
    notes = [l.split("\t")[-1] for l in want_out.splitlines()[1:]]
    assert any("af-filter" in n for n in notes) and any(("missing-data-error" if model == "fixed" else "lrt-filtering-failed") in n for n in notes)
