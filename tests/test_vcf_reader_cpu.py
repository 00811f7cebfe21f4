"""VCF and burden input through the text reader (pyseer_amd/input.py: open_variant_file / read_variant / load_burden; the reference's
pyseer/input.py:250-266, 383-407, 455-503).  Runs without a GPU.

The expectations are (1) facts about the reference's own data files (tests/golden/vcf/facts.json) and (2) hand-written files whose
expected values are worked out by hand from the rules in DESIGN.md ("VCF input"): a sample is present as soon as one GT haplotype is a non-zero
allele, otherwise missing if its last haplotype is `.`, absent if it is `0`; a burden variant is present where any of its records is, otherwise
what the last applied record says."""
import collections
import gzip
import json
import math
import os

import numpy as np
import pandas as pd
import pytest

from pyseer_amd.input import load_burden, open_variant_file, read_variant

from _vcf_text import generated_vcf, write_bgzf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VCF = os.path.join(ROOT, "tests", "golden", "vcf")
FACTS = json.load(open(os.path.join(VCF, "facts.json")))


def _pheno():
    p = pd.read_csv(os.path.join(ROOT, "tests", "golden", "cli", "subset.pheno"), index_col=0, sep="\t")["binary"]
    p.index = p.index.astype(str)
    return p


def _read(infile, p, burden=False, regions=None):
    return read_variant(infile, p, "vcf", burden, regions, False, set(p.index), [])


def _same_k(k, want):
    k, want = np.asarray(k, dtype=float), np.asarray(want, dtype=float)
    return k.shape == want.shape and bool(np.all((k == want) | (np.isnan(k) & np.isnan(want))))


def _all_tuples(path, p):
    infile, order = open_variant_file("vcf", path)
    out = []
    while True:
        t = _read(infile, p)
        if t[0]:
            return out
        out.append(t)


# ---- 1. the recorded facts ---------------------------------------------------------------------------------------------------------------
def test_first_record_of_the_subset(capsys):
    f = FACTS["first_record"]
    p = _pheno()
    infile, order = open_variant_file("vcf", os.path.join(VCF, f["vcf"]))
    assert order == []
    assert set(p.index) <= set(infile.samples) and list(p.index) != [s for s in infile.samples if s in set(p.index)]   # another column order
    assert len(set(infile.samples) - set(p.index)) >= 3                                                              # columns without phenotype
    eof, k, name, ks, nks, af, missing = _read(infile, p)
    assert (eof, name, ks, af, missing) == (False, f["name"], f["kstrains"], f["af"], f["missing"])
    assert nks == sorted(p.index) and k.shape == (50,) and not k.any()
    assert "No observations of %s in selected samples" % f["name"] in capsys.readouterr().err
    # the second record has two ALT alleles: no name, nothing else
    assert _read(infile, p) == (False, None, None, None, None, None, None)
    assert capsys.readouterr().err == "Multiple alleles at FM211187_23. Skipping\n"


def test_first_record_over_all_samples(capsys):
    f = FACTS["first_record_all_samples"]
    infile, _ = open_variant_file("vcf", os.path.join(VCF, f["vcf"]))
    assert len(infile.samples) == 1837
    p = pd.Series(np.zeros(len(infile.samples)), index=infile.samples)
    eof, k, name, ks, nks, af, missing = _read(infile, p)
    assert name == f["name"]
    assert ks == sorted(f["present"] + f["missing"])
    assert [s for s, v in zip(p.index, k) if v == 1] == sorted(f["present"], key=list(p.index).index)
    assert [s for s, v in zip(p.index, k) if np.isnan(v)] == f["missing"]
    assert af == 11 / 1837.0 and missing == 1 / 1837.0
    capsys.readouterr()
    names = [_read(infile, p)[2] for _ in range(2)]
    assert [name] + names == f["records"]
    assert capsys.readouterr().err == f["stderr"]
    assert _read(infile, p)[0] is True                                   # end of file: eof, and again
    assert _read(infile, p) == (True, None, None, None, None, None, None)


@pytest.mark.parametrize("case", range(len(FACTS["burden_first_five"])))
def test_burden_over_the_first_five_samples(case):
    f = FACTS["burden_first_five"][case]
    p = _pheno().head(5)
    regions = collections.deque()
    infile, _ = open_variant_file("vcf", os.path.join(VCF, f["vcf"]), os.path.join(VCF, f["regions"]), regions)
    for _ in range(f["take"]):
        regions.popleft()
    eof, k, name, ks, nks, af, missing = _read(infile, p, True, regions)
    assert (eof, name, ks, af, missing) == (False, f["name"], f["kstrains"], f["af"], f["missing"])
    assert _same_k(k, f["k"]) and nks == sorted(set(p.index) - set(ks))


def test_burden_regions_of_the_subset():
    f = FACTS["burden_50"]
    p = _pheno()
    regions = collections.deque()
    infile, _ = open_variant_file("vcf", os.path.join(VCF, f["vcf"]), os.path.join(VCF, f["regions"]), regions)
    assert list(regions) == [("CDS1", ["FM211187:3910-3951"]), ("CDS2", ["FM211187:4006-4057"]),
                             ("CDS3", ["FM211187:3910-3951", "FM211187:4006-4057"])]
    got = {}
    while True:
        t = _read(infile, p, True, regions)
        if t[0]:
            break
        got[t[2]] = t[5]
    assert list(got) == ["CDS1", "CDS2", "CDS3"] and got == f["af"]


def test_format_without_gt_is_all_missing():
    f = FACTS["no_gt"]
    p = _pheno()
    infile, _ = open_variant_file("vcf", os.path.join(VCF, f["vcf"]))
    eof, k, name, ks, nks, af, missing = _read(infile, p)
    assert (name, af, missing, nks) == (f["name"], f["af"], f["missing"], []) and np.isnan(k).all() and ks == sorted(p.index)


def test_counts_of_the_subset(capsys):
    f = FACTS["counts_50"]
    ts = _all_tuples(os.path.join(VCF, f["vcf"]), _pheno())
    err = capsys.readouterr().err.splitlines()
    want = open(os.path.join(VCF, "lmm50_expected.err")).read().splitlines()
    assert len(ts) == f["records"] and sum(t[2] is None for t in ts) == f["skipped"]
    assert sum(l.startswith("Multiple alleles") for l in err) == f["multiallelic"]
    assert [l for l in err if l.startswith("Multiple")] == [l for l in want if l.startswith("Multiple")]
    assert [l for l in err if l.startswith("No obs")] == [l for l in want if l.startswith("No obs")] and len([l for l in err if l.startswith("No obs")]) == f["no_observations"]
    rows = open(os.path.join(VCF, "lmm50_expected.log")).read().splitlines()[1:]
    seen = [t for t in ts if t[2] is not None and t[5] > 0]
    assert [t[2] for t in seen] == [r.split("\t")[0] for r in rows] and len(seen) == f["observed"]
    assert ["%.2E" % t[5] for t in seen] == [r.split("\t")[1] for r in rows]       # af as the reference's recorded run printed it


def test_missing_fraction_of_variants_missing():
    """The fraction of missing calls among the phenotyped samples, counted straight from the text of the first record."""
    p = _pheno()
    path = os.path.join(VCF, "variants_missing.vcf.gz")
    with gzip.open(path, "rt") as fh:
        lines = [l for l in fh if not l.startswith("##")]
    cols = lines[0].rstrip("\n").split("\t")
    rec = lines[1].rstrip("\n").split("\t")
    n_missing = sum(1 for c, f in zip(cols[9:], rec[9:]) if c in set(p.index) and f.split(":")[0] == ".")
    infile, _ = open_variant_file("vcf", path)
    t = _read(infile, p)
    assert n_missing > 0 and t[6] == n_missing / 50.0 and int(np.isnan(t[1]).sum()) == n_missing


# ---- 2. the three-way code, every GT form ---------------------------------------------------------------------------------------------------
GT_FORMS = [("0", 0), ("1", 1), (".", None), ("0/1", 1), ("./.", None), ("./1", 1), ("0/.", None), ("./0", 0), ("1|0", 1), ("2", 1),
            ("", None), ("0|0", 0), (".|.", None), ("10", 1)]
COLS = ["c%02d" % i for i in range(len(GT_FORMS))]


def _hand_vcf(tmp_path):
    gts = [g for g, _ in GT_FORMS]
    head = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(COLS + ["nopheno"])
    rec = lambda pos, ref, alt, flt, fmt, fields: "\t".join(["chrA", str(pos), ".", ref, alt, "9", flt, "X=1", fmt] + fields)
    lines = [head,
             rec(5, "A", "T", "PASS", "GT", gts + ["1"]),                                                 # GT alone
             rec(6, "A", "T", ".", "DP:GT:GQ", ["7:%s:9" % g for g in gts[:-1]] + ["7", "3:1:1"]),          # GT second; the last phenotyped field stops before GT
             rec(7, "AC", "A", "PASS", "DP:GQ", ["7:9"] * (len(gts) + 1)),                                # no GT at all
             rec(8, "G", ".", "q10;PASS", "GT:DP", ["0:1"] * 3 + ["1:1"] + ["0:1"] * (len(gts) - 3)),      # ALT '.', a filter list that holds PASS
             rec(9, "G", "A", "q10", "GT", ["1"] * (len(gts) + 1)),                                       # filtered
             rec(10, "G", "A,T", "PASS", "GT", ["1"] * (len(gts) + 1)),                                   # two ALT alleles
             rec(11, "G", "A", "LowQual;q10", "GT", ["1"] * (len(gts) + 1)),                              # filtered
             rec(12, "G", "C", "PASS", "GT", ["0"] * (len(gts) + 1))]                                     # nobody
    path = tmp_path / "hand.vcf"
    path.write_text("\n".join(lines))                                                                     # (no newline after the last record)
    return str(path)


def test_three_way_code_on_every_gt_form(tmp_path, capsys):
    path = _hand_vcf(tmp_path)
    # phenotype order differs from the column order; `absent_everywhere` is in no VCF column; `nopheno` has no phenotype
    order = COLS[::-1] + ["absent_everywhere"]
    p = pd.Series(np.arange(len(order)) % 2, index=order)
    ts = _all_tuples(path, p)
    err = capsys.readouterr().err
    n = float(len(order))
    nan = float("nan")
    want_k = [nan if c is None else c for _, c in GT_FORMS]
    present_or_missing = sorted(c for c, (_, code) in zip(COLS, GT_FORMS) if code != 0)
    # record 1
    eof, k, name, ks, nks, af, missing = ts[0]
    assert name == "chrA_5_A_T" and _same_k(k, want_k[::-1] + [0])
    assert ks == present_or_missing and nks == sorted(set(order) - set(ks))
    assert af == len(ks) / n and missing == sum(c is None for _, c in GT_FORMS) / n
    # record 2: GT second in FORMAT gives the same codes; the field that ends before GT is missing
    k2 = want_k[:-1] + [nan]
    assert ts[1][2] == "chrA_6_A_T" and _same_k(ts[1][1], k2[::-1] + [0])
    # record 3: no GT -> every VCF sample missing, the sample the VCF does not have absent
    assert ts[2][2] == "chrA_7_AC_A" and _same_k(ts[2][1], [nan] * len(COLS) + [0]) and ts[2][5] == len(COLS) / n and ts[2][6] == len(COLS) / n
    # record 4: ALT '.' -> CHROM_POS_REF; FILTER q10;PASS is kept
    assert ts[3][2] == "chrA_8_G" and ts[3][3] == ["c03"] and ts[3][5] == 1 / n and ts[3][6] == 0.0
    # records 5-7: skipped
    none = (False, None, None, None, None, None, None)
    assert ts[4] == none and ts[5] == none and ts[6] == none
    # record 8 (no newline at the end of the file): nobody carries it
    assert ts[7][2] == "chrA_12_G_C" and ts[7][3] == [] and ts[7][5] == 0.0 and not ts[7][1].any() and len(ts) == 8
    assert err == "Multiple alleles at chrA_10. Skipping\nNo observations of chrA_12_G_C in selected samples\n"


# ---- 3. burden ------------------------------------------------------------------------------------------------------------------------------
def _burden_files(tmp_path):
    head = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts1\ts2\ts3\n"
    recs = [("chr1", 10, "A", "T", "PASS", [".", "0", "0"]),
            ("chr1", 18, "ACGTA", "A", "PASS", ["0", "1", "0"]),           # a deletion over [17, 22): starts before chr1:20-30, reaches into it
            ("chr1", 20, "C", "T", "PASS", ["0", "0", "."]),
            ("chr1", 30, "G", "A", "PASS", ["0", "0", "0"]),
            ("chr1", 40, "G", "A,C", "PASS", ["1", "1", "1"]),             # skipped: contributes nothing
            ("chr1", 50, "T", "C", "PASS", ["0", ".", "0"]),
            ("chr1", 60, "T", "C", "q10", ["1", "1", "1"]),                # skipped: contributes nothing
            ("chr2", 10, "A", "G", "PASS", ["1", "0", "0"])]
    vcf = tmp_path / "burden.vcf"
    vcf.write_text(head + "".join("\t".join([c, str(pos), ".", ref, alt, "9", flt, ".", "GT"] + gt) + "\n" for c, pos, ref, alt, flt, gt in recs))
    regions = tmp_path / "regions.txt"
    regions.write_text("G1 chr1:20-30\nG2 chr1:25-50\nG3 chr1:10-10,chr1:10-10\nG4 chr1:100-200\nG5 chr1:5,chr2:10-10\n"
                       "G6 chr1:10-10,chr1:50-50\nG7 chr1:50-50,chr1:10-10\nG8 chr1:55-65\n")
    return str(vcf), str(regions)


nan_ = float("nan")
BURDEN_WANT = [("G1", [0, 1, 0]),            # 18: s2 present; 20: s3 missing; 30: s3 reference again -> absent
               ("G2", [0, nan_, 0]),         # overlaps G1 (record 30 serves both); 40 skipped; 50 last: s2 missing
               ("G3", [nan_, 0, 0]),         # the same region twice
               ("G4", [0, 0, 0]),            # no record
               ("G5", [1, 0, 0]),            # an unparsable region, then chr2
               ("G6", [0, nan_, 0]),         # s1: missing then reference -> absent; s2: reference then missing -> missing
               ("G7", [nan_, 0, 0]),         # the other order
               ("G8", [0, 0, 0])]            # only a filtered record


def test_burden_rules(tmp_path, capsys):
    vcf, reg = _burden_files(tmp_path)
    p = pd.Series([0, 1, 0], index=["s1", "s2", "s3"])
    regions = collections.deque()
    infile, _ = open_variant_file("vcf", vcf, reg, regions)
    assert len(regions) == 8
    got = []
    while True:
        t = _read(infile, p, True, regions)
        if t[0]:
            break
        got.append(t)
    assert [t[2] for t in got] == [n for n, _ in BURDEN_WANT]
    for t, (name, k) in zip(got, BURDEN_WANT):
        assert _same_k(t[1], k), (name, t[1])
        carriers = [s for s, v in zip(p.index, k) if v != 0]
        assert t[3] == carriers and t[4] == [s for s in p.index if s not in carriers], name
        assert t[5] == len(carriers) / 3.0 and t[6] == sum(1 for v in k if math.isnan(v)) / 3.0, name
    assert capsys.readouterr().err == ("Multiple alleles at chr1_40. Skipping\nNo observations of G4 in selected samples\n"
                                       "Could not parse region None\nNo observations of G8 in selected samples\n")
    # load_burden alone
    lst = []
    load_burden(reg, lst)
    assert lst[2] == ("G3", ["chr1:10-10", "chr1:10-10"]) and lst[4] == ("G5", ["chr1:5", "chr2:10-10"])


# ---- 4. containers --------------------------------------------------------------------------------------------------------------------------
def test_plain_gzip_and_bgzf_give_the_same_tuples(tmp_path, capsys):
    text, pheno, cols = generated_vcf(n_pheno=40, n_cols=47, n_records=120, seed=11)
    paths = [str(tmp_path / n) for n in ("g.vcf", "g.vcf.gz", "g.bgzf.vcf.gz")]
    open(paths[0], "wb").write(text)
    with gzip.open(paths[1], "wb") as f:
        f.write(text)
    write_bgzf(paths[2], text)
    assert open(paths[2], "rb").read(16)[12:14] == b"BC" and gzip.open(paths[2], "rb").read() == text
    p = pd.Series(np.arange(40) % 2, index=pheno)
    runs = []
    for path in paths:
        ts = _all_tuples(path, p)
        runs.append(([(t[0], t[2], t[3], t[4], t[5], t[6]) for t in ts], [None if t[1] is None else t[1].tolist() for t in ts], capsys.readouterr().err))
    assert len(runs[0][0]) == 120 and any(t[1] is None for t in runs[0][0]) and any(t[5] for t in runs[0][0] if t[1])
    assert repr(runs[0]) == repr(runs[1]) == repr(runs[2])
