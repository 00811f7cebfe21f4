#!/usr/bin/env python3
"""VCF fixtures under tests/golden/vcf/, cut from the reference's own test DATA files (no program of the reference is read or run).

    python tests/golden/make_vcf_fixtures.py <directory of the reference's tests>

 variants50.vcf.gz      variants_smaller.vcf.gz (254 records x 1837 samples) cut to the 50 samples of cli/subset.pheno plus five that have no
                        phenotype, the columns written in another order than the phenotype's; BGZF
 variants_head.vcf.gz   the header and the first three records of variants_smaller.vcf.gz (a kept one, a multi-allelic one, a kept one) over all
                        1837 samples
 variants_missing.vcf.gz, variants_no_gt.vcf.gz, burden_regions.txt, burden_regions_multiple.txt, burden_missing.txt: as they are
 lmm50_expected.log/.err  the rows of the reference's recorded run tests/baseline/23.log (--vcf variants.vcf.gz --phenotypes subset.pheno
                        --lmm --load-lmm ...) and the `No observations` lines of 23.err whose names are records of variants50.vcf.gz, in
                        the small file's order, plus the `Multiple alleles` lines and the four counters the subset implies
 burden_expected.tsv    variant, af, filter-pvalue of tests/baseline/13.log and 37.log (the other columns depend on a projection whose
                        distance file is not shipped)
"""
import gzip
import os
import shutil
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from _vcf_text import write_bgzf  # noqa: E402

REF = sys.argv[1]
OUT = os.path.join(HERE, "vcf")
os.makedirs(OUT, exist_ok=True)

for f in ("variants_missing.vcf.gz", "variants_no_gt.vcf.gz", "burden_regions.txt", "burden_regions_multiple.txt", "burden_missing.txt"):
    shutil.copy(os.path.join(REF, f), os.path.join(OUT, f))
    os.chmod(os.path.join(OUT, f), 0o644)

pheno = [l.split("\t")[0] for l in open(os.path.join(HERE, "cli", "subset.pheno")).read().splitlines()[1:]]
extra = ["sample_1647", "sample_60", "sample_999", "sample_1837", "sample_51"]
# another order than the phenotype's: the extras spread among the phenotyped samples taken back to front in strides of 7
order = [pheno[(i * 7) % len(pheno)] for i in range(len(pheno))][::-1]
for j, e in enumerate(extra):
    order.insert(3 + 11 * j, e)
out, names, skipped, head = [], [], [], []
with gzip.open(os.path.join(REF, "variants_smaller.vcf.gz"), "rt") as fh:
    for line in fh:
        if line.startswith("#") or len(head) < 3 + sum(1 for x in head if x.startswith("#")):
            head.append(line)
        if line.startswith("##"):
            out.append(line)
            continue
        f = line.rstrip("\n").split("\t")
        if line.startswith("#"):
            col = {name: i for i, name in enumerate(f)}
            take = [col[s] for s in order]
        else:
            alts = f[4].split(",")
            flt = [x for x in f[6].split(";") if x not in (".", "")]
            if len(alts) > 1:
                skipped.append("Multiple alleles at %s_%s. Skipping" % (f[0], f[1]))
            elif not (flt and "PASS" not in flt):
                names.append("_".join([f[0], f[1], f[3]] + ([] if f[4] == "." else alts)))
        out.append("\t".join(f[:9] + [f[i] for i in take]) + "\n")
write_bgzf(os.path.join(OUT, "variants_head.vcf.gz"), "".join(head).encode(), level=9)
write_bgzf(os.path.join(OUT, "variants50.vcf.gz"), "".join(out).encode(), level=9)

log = open(os.path.join(REF, "baseline", "23.log")).read().splitlines()
err = open(os.path.join(REF, "baseline", "23.err")).read().splitlines()
row_of = {l.split("\t")[0]: l for l in log[1:]}
noobs = set(l[len("No observations of "):-len(" in selected samples")] for l in err if l.startswith("No observations of "))
rows, errs = [], []
for n in names:
    assert (n in row_of) != (n in noobs), n
    if n in row_of:
        rows.append(row_of[n])
    else:
        errs.append("No observations of " + n + " in selected samples")
nrec = sum(1 for l in out if not l.startswith("#"))
with open(os.path.join(OUT, "lmm50_expected.log"), "w") as f:
    f.write("\n".join([log[0]] + rows) + "\n")
with open(os.path.join(OUT, "lmm50_expected.err"), "w") as f:
    f.write("\n".join(skipped) + "\n" + "\n".join(errs) + "\n")
    f.write("%d loaded variants\n%d pre-filtered variants\n%d tested variants\n%d printed variants\n"
            % (nrec, nrec - len(rows), len(rows), len(rows)))
b13 = [l.split("\t")[:3] for l in open(os.path.join(REF, "baseline", "13.log")).read().splitlines()]
b37 = [l.split("\t")[:3] for l in open(os.path.join(REF, "baseline", "37.log")).read().splitlines()]
assert b13[1:] == b37[1:3]
with open(os.path.join(OUT, "burden_expected.tsv"), "w") as f:
    f.write("".join("\t".join(r) + "\n" for r in b37))
print(nrec, "records,", len(names), "kept names,", len(rows), "rows,", len(errs), "without observations,", len(skipped), "multi-allelic")
