"""BCF input on the device: k_bcf_gt_pack (csrc/vcf_kernels.hip) against the library's host restatement and against the text route's
k_vcf_gt_pack on the same records, and the command line, --wg enet and similarity on a converted fixture against their runs on the text file.
The BCF files are written at test time by tests/_bcf_bytes.py."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

from _bcf_bytes import WORKED_HEADER, bcf_from_vcf_text  # noqa: E402
from _bcf_check import assert_same, native_records  # noqa: E402
from _vcf_text import bgzf_bytes, generated_vcf  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "golden", "cli")
VCF = os.path.join(ROOT, "tests", "golden", "vcf")
V50 = os.path.join(VCF, "variants50.vcf.gz")
BLOCKS = (1, 7, 3000)


def _write(path, data):
    with open(str(path), "wb") as f:
        f.write(data)
    return str(path)


def _three_routes(text, samples, tmp_path, **how):
    """k_bcf_gt_pack at every block size = the host restatement = k_vcf_gt_pack on the text of the same records."""
    from pyseer_amd.engine import Engine
    tpath = _write(tmp_path / "t.vcf.gz", bgzf_bytes(text, level=1))
    bpath = _write(tmp_path / "t.bcf", bcf_from_vcf_text(text, **how))
    host = native_records(bpath, samples, None, 3000)
    e = Engine(len(samples))
    try:
        text_rows = native_records(tpath, samples, e, 3000)
        assert "format" not in text_rows[8]
        assert_same(host, text_rows, "host restatement of BCF against k_vcf_gt_pack on text")
        for bs in BLOCKS:
            got = native_records(bpath, samples, e, bs)
            assert got[8]["format"] == "bcf"
            assert_same(got, host, "k_bcf_gt_pack against the host restatement, block size %d" % bs)
            assert_same(got, text_rows, "k_bcf_gt_pack against k_vcf_gt_pack, block size %d" % bs)
            assert np.array_equal(got[6], text_rows[6]) and np.array_equal(got[7], text_rows[7])       # POS, len(REF)
    finally:
        e.close()
    return host


# 63/70: one partial word; 64/64: the row exactly full, every column phenotyped; 65/300 and 257/520: more columns than one stride of 256 lanes
@pytest.mark.parametrize("n_pheno,n_cols", [(63, 70), (64, 64), (65, 300), (257, 520)])
def test_kernel_equals_host_restatement_and_text_kernel(n_pheno, n_cols, tmp_path):
    text, pheno, cols = generated_vcf(n_pheno=n_pheno, n_cols=n_cols, n_records=200, seed=n_cols, missing=0.04)
    rows = _three_routes(text, pheno, tmp_path, idx=(n_cols % 2 == 0))
    skip = rows[1].tolist()
    assert len(skip) == 200 and skip.count(1) > 0 and skip.count(2) > 0 and rows[4].sum() > 0 and rows[5].sum() > 0


def _hand_made(n_cols=300):
    """Records of ploidy three (L = 3) with every kind of call at every place of the vector, beside haploid and empty ones."""
    rng = np.random.RandomState(3)
    calls = ["0/0/0", "0/0/1", "1/0/0", "0|1|0", "./0/0", "0/0/.", "././.", "./1/.", "0/./0", "0", "1", ".", "", "0/0", "./1", "1|."]
    cols = ["c%03d" % i for i in range(n_cols)]
    lines = [WORKED_HEADER.split("#CHROM")[0] + "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(cols)]
    for r in range(40):
        f = [calls[i] for i in rng.randint(len(calls), size=n_cols)]
        fmt = "GT"
        if r % 3 == 1:
            fmt, f = "DP:GT", [("%d:%s" % (rng.randint(300), x) if x else "") for x in f]
        lines.append("\t".join(["chr1", str(10 + r), ".", "A", "G", ".", "PASS", ".", fmt] + f))
    pheno = [cols[i] for i in rng.permutation(n_cols)[:257]]
    return ("\n".join(lines) + "\n").encode(), pheno


@pytest.mark.parametrize("how", [{}, {"gt_int16": True}, {"gt_last": True, "gt_int16": True}])
def test_ploidy_three_and_int16_gt(how, tmp_path):
    text, pheno = _hand_made()
    rows = _three_routes(text, pheno, tmp_path, **how)
    assert rows[4].min() > 0 and rows[5].min() > 0


# ---- the command line ---------------------------------------------------------------------------------------------------------------------------
def _cli(args, module="pyseer_amd"):
    env = dict(os.environ); env["PYTHONPATH"] = ROOT
    r = subprocess.run([sys.executable, "-m", module] + args, cwd=CLI, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return r.stdout.decode(), r.stderr.decode()


@pytest.fixture(scope="module")
def v50_bcf(tmp_path_factory):
    return _write(tmp_path_factory.mktemp("bcf") / "variants50.bcf", bcf_from_vcf_text(gzip.open(V50).read(), idx=True))


MODELS = {"fixed": ["--distances", "distances50.tsv"], "lmm": ["--similarity", "similarity50.tsv", "--lmm"],
          "burden": ["--burden", os.path.join(VCF, "burden_regions_multiple.txt"), "--no-distances"]}
_text_runs = {}


def _text_run(model):
    if model not in _text_runs:
        _text_runs[model] = _cli(["--vcf", V50, "--phenotypes", "subset.pheno", "--print-samples"] + MODELS[model])
    return _text_runs[model]


@pytest.mark.parametrize("reader", [[], ["--python-reader"]])
@pytest.mark.parametrize("model", ["fixed", "lmm", "burden"])
def test_cli_on_bcf_is_byte_identical_to_cli_on_text(model, reader, v50_bcf):
    out, err = _cli(["--vcf", v50_bcf, "--phenotypes", "subset.pheno", "--print-samples"] + MODELS[model] + reader)
    want = _text_run(model)
    assert out == want[0] and len(out.splitlines()) > 1
    assert err == want[1]


def test_similarity_on_bcf_equals_similarity_on_text(v50_bcf):
    samples = os.path.join(CLI, "samples50.txt")
    want = _cli([samples, "--vcf", V50], module="pyseer_amd.similarity")
    assert _cli([samples, "--vcf", v50_bcf], module="pyseer_amd.similarity") == want
    assert _cli([samples, "--vcf", v50_bcf, "--python-reader"], module="pyseer_amd.similarity") == want


# the fit replaced by a fixed slope vector, as tests/test_enet_vcf_native_gpu.py does: what is compared is everything the reader feeds
_FIXED = ("import sys, numpy as np\n"
          "from pyseer_amd import enet\n"
          "def fixed_betas(n_cov, var_indices):\n"
          "    j = np.arange(len(var_indices))\n"
          "    return np.concatenate([[0.25], np.zeros(n_cov), np.where(j % 7 == 0, ((j * 37) % 11 - 5) / 10.0 + 0.05, 0.0)])\n"
          "enet.TEST_BETAS = fixed_betas\n"
          "from pyseer_amd.__main__ import main\n"
          "main(sys.argv[1:])\n"
          "sys.stderr.write('route %s\\n' % getattr(enet, 'LAST_LOAD_ROUTE', None))\n")


@pytest.mark.parametrize("extra", [[], ["--burden", os.path.join(VCF, "burden_regions_multiple.txt")]])
def test_wg_enet_on_bcf_equals_wg_enet_on_text(extra, v50_bcf):
    runs = []
    for path in (V50, v50_bcf):
        r = subprocess.run([sys.executable, "-c", _FIXED, "--vcf", path, "--phenotypes", "subset.pheno", "--min-af", "0.05", "--max-af", "0.95", "--wg", "enet",
                            "--phenotype-column", "binary"] + extra, cwd=CLI, env=dict(os.environ, PYTHONPATH=ROOT), stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, timeout=600)
        assert r.returncode == 0, r.stderr.decode()[-3000:]
        runs.append((r.stdout.decode(), r.stderr.decode()))
    assert runs[0] == runs[1] and len(runs[0][0].splitlines()) > 1 and runs[0][1].endswith("route calls\n")
