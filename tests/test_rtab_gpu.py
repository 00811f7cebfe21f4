"""The native Rtab reader on the device (sh_rtab_*, k_rtab_pack; csrc/rtab_kernels.hip).

1. The kernel against its host restatement (shrtab::host_rtab_pack, the reader opened without an engine), bit for bit: status, rows, counts,
   with one wavefront and with one workgroup per line (SEERHIP_ROUTE rtab_wg), over column counts around every power of the partition and
   lines whose byte length falls on and beside each of the kernel's own boundaries (sh_rtab_partition).
2. The command lines that take --pres: the default (native) run and --python-reader print the same bytes.
3. The call-block stream into the whole-genome loader against the reference's golden rows; enet_predict and malformed lines; --gpus."""
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "golden", "cli")
ENET = os.path.join(ROOT, "tests", "golden", "enet")
PREDICT = os.path.join(ROOT, "tests", "golden", "predict")
ROWS = 40
KEYS = ("status", "present", "missing", "n_present", "n_missing", "off")


# ---- 1. kernel = host restatement --------------------------------------------------------------------------------------------------------
def _columns(n_cols, rng):
    """(file columns, phenotype samples): the phenotype in another order, one sample without a column, two columns without a phenotype"""
    cols = ["c%d" % i for i in range(n_cols)]
    drop = set(rng.choice(n_cols, size=2, replace=False).tolist()) if n_cols > 3 else set()
    pheno = [c for i, c in enumerate(cols) if i not in drop] + ["nocolumn"]
    return cols, [pheno[i] for i in rng.permutation(len(pheno))]


def _calls(n_cols, rng, empties=None):
    """n_cols calls, the last never empty; empties: exactly that many empty calls (the byte length is then 2 * n_cols - 1 - empties)"""
    if empties is None:
        calls = [("0", "1", ".", "")[i] for i in rng.choice(4, size=n_cols, p=[0.4, 0.4, 0.1, 0.1])]
        if calls[-1] == "":
            calls[-1] = "."
        return calls
    calls = [("0", "1", ".")[i] for i in rng.choice(3, size=n_cols, p=[0.45, 0.45, 0.1])]
    for i in rng.choice(n_cols - 1, size=empties, replace=False):
        calls[i] = ""
    return calls


def _write(path, cols, rows):
    with open(path, "wb") as f:
        f.write(("Gene\t" + "\t".join(cols) + "\n").encode())
        for i, calls in enumerate(rows):
            f.write((("g%d" % i) + ("\t" + "\t".join(calls) if calls is not None else "") + "\n").encode())


def _read_all(path, pheno, engine, block_size):
    from pyseer_amd.input import NativeRtabReader
    r = NativeRtabReader(path, pheno, engine, block_size)
    try:
        blocks = list(r.raw_blocks())
        stats, part = r.stats(), r.partition()
    finally:
        r.close()
    out = {k: np.concatenate([b[k] if k != "off" else np.diff(b[k]) for b in blocks]) for k in KEYS}
    out["blob"] = b"".join(b["blob"] for b in blocks)
    return out, stats, part


def _assert_device_equals_host(path, pheno, engine, monkeypatch, block_size=3000, route=""):
    want, _, _ = _read_all(path, pheno, None, block_size)
    stats = {}
    for wg in (64, 256):
        monkeypatch.setenv("SEERHIP_ROUTE", "rtab_wg=%d%s" % (wg, route))
        got, stats[wg], part = _read_all(path, pheno, engine, block_size)
        assert part["step"] == wg * part["lane"]
        assert stats[wg]["launches"] > 0
        for k in KEYS + ("blob",):
            assert np.array_equal(got[k], want[k]) if k != "blob" else got[k] == want[k], (wg, k)
    monkeypatch.delenv("SEERHIP_ROUTE")
    return want, stats


@pytest.mark.parametrize("n_cols", [1, 2, 7, 8, 9, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4100])
def test_kernel_equals_host_restatement(n_cols, tmp_path, monkeypatch):
    from pyseer_amd.engine import Engine
    rng = np.random.default_rng(n_cols)
    cols, pheno = _columns(n_cols, rng)
    rows = [_calls(n_cols, rng) for _ in range(ROWS)]
    rows[5] = None                                                        # status 1
    rows[9] = rows[9][:-1] if n_cols > 1 else ["1", "0"]                  # status 2
    rows[13][rng.integers(n_cols)] = "2"                                  # status 3
    rows[17][n_cols // 2] = "01"
    rows[21] = ["0"] * n_cols
    path = str(tmp_path / "t.Rtab")
    _write(path, cols, rows)
    e = Engine(len(pheno))
    try:
        want, _ = _assert_device_equals_host(path, pheno, e, monkeypatch)
    finally:
        e.close()
    assert [int(want["status"][i]) for i in (5, 9, 13, 17, 21)] == [1, 2, 3, 3, 0]
    assert (want["status"] == 0).sum() == ROWS - 4 and want["n_present"].sum() > 0


def _partition(engine, pheno, path, monkeypatch, wg):
    from pyseer_amd.input import NativeRtabReader
    monkeypatch.setenv("SEERHIP_ROUTE", "rtab_wg=%d" % wg)
    r = NativeRtabReader(path, pheno, engine, 1)
    try:
        return r.partition()
    finally:
        r.close()
        monkeypatch.delenv("SEERHIP_ROUTE")


def test_line_ends_and_bad_tokens_on_the_kernels_boundaries(tmp_path, monkeypatch):
    """Per boundary B of the kernel's partition (a lane's bytes, a wavefront's span, a step of either launch shape, two steps): lines of B - 1,
    B and B + 1 bytes of call text (empty calls take the bytes out), and a two-byte token that lies across B (status 3: either half alone
    would be a call)."""
    from pyseer_amd.engine import Engine
    rng = np.random.default_rng(5)
    probe = str(tmp_path / "probe.Rtab")
    _write(probe, ["c0", "c1"], [["1", "0"]])
    e2 = Engine(3)
    try:
        parts = [_partition(e2, ["c0", "c1", "nocolumn"], probe, monkeypatch, wg) for wg in (64, 256)]
    finally:
        e2.close()
    bounds = sorted({parts[0]["lane"], parts[0]["wave"], parts[0]["step"], parts[1]["step"], 2 * parts[0]["step"], 2 * parts[1]["step"]})
    assert bounds[0] == 16 and all(b % 2 == 0 for b in bounds)
    for B in bounds:
        n_cols = B // 2 + 3                                               # 2 * n_cols - 1 = B + 5 bytes without an empty call
        cols, pheno = _columns(n_cols, rng)
        rows, lengths = [], []
        for r in range(ROWS):
            if r % 4 == 3:                                                # an empty first call moves call i to byte 2 i - 1: call B / 2 starts at B - 1
                calls = _calls(n_cols, rng, 0)
                calls[0] = ""
                calls[B // 2] = "10"
                lengths.append(None)
            else:
                want_len = B - 1 + r % 4
                calls = _calls(n_cols, rng, 2 * n_cols - 1 - want_len)
                lengths.append(want_len)
            rows.append(calls)
            text = "\t".join(calls)
            assert lengths[-1] in (None, len(text)) and (lengths[-1] is not None or text[B - 1:B + 1] == "10")
        path = str(tmp_path / ("b%d.Rtab" % B))
        _write(path, cols, rows)
        e = Engine(len(pheno))
        try:
            want, _ = _assert_device_equals_host(path, pheno, e, monkeypatch)
        finally:
            e.close()
        assert [int(s) for s in want["status"]] == [3 if r % 4 == 3 else 0 for r in range(ROWS)]


def test_slabs_grow_and_block_sizes(tmp_path, monkeypatch):
    from pyseer_amd.engine import Engine
    rng = np.random.default_rng(11)
    # lines of ~8 KB against slabs of 4 KB: the first line makes the slabs grow, later sub-batches fill them
    cols, pheno = _columns(4100, rng)
    path = str(tmp_path / "grow.Rtab")
    _write(path, cols, [_calls(4100, rng) for _ in range(ROWS)])
    e = Engine(len(pheno))
    try:
        _, stats = _assert_device_equals_host(path, pheno, e, monkeypatch, route=",rtab_slab=4096")
        assert stats[64]["launches"] > 4                                  # (one 32 MB slab would have taken the file in one launch)
    finally:
        e.close()
    cols, pheno = _columns(65, rng)
    path = str(tmp_path / "small.Rtab")
    _write(path, cols, [_calls(65, rng) for _ in range(ROWS)])
    e = Engine(len(pheno))
    try:
        for bs in (1, 7, 3000):                                           # one line per call; blocks that end inside the file; one larger than it
            _, stats = _assert_device_equals_host(path, pheno, e, monkeypatch, block_size=bs)
            assert stats[256]["rows"] == ROWS and stats[256]["launches"] == -(-ROWS // bs)
    finally:
        e.close()


# ---- 2. the command lines ----------------------------------------------------------------------------------------------------------------
def _cli(args, module="pyseer_amd", expect=0):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", module] + args, cwd=CLI, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == expect, r.stderr.decode()[-3000:]
    return r.stdout.decode(), r.stderr.decode()


MARKED = ("import sys; from pyseer_amd.__main__ import main; from pyseer_amd import input as I\n"
          "try:\n    main(sys.argv[1:])\nfinally:\n    sys.stdout.flush(); sys.stderr.write('\\nRTAB_LAUNCHES=%s\\n' % I.LAST_RTAB_LAUNCHES)\n")


def _cli_marked(args):
    """the command line in a process of its own that says at its end how many kernel launches its Rtab reader made (input.LAST_RTAB_LAUNCHES)"""
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", MARKED] + args, cwd=CLI, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    err, _, mark = r.stderr.decode().rpartition("\nRTAB_LAUNCHES=")
    return r.stdout.decode(), err, mark.strip()


PRES = ["--pres", "kmers120.Rtab", "--phenotypes", "subset.pheno"]
RUNS = [("fixed", ["--distances", "distances50.tsv"]),
        ("lmm", ["--similarity", "similarity50.tsv", "--lmm"]),
        ("lineage", ["--distances", "distances50.tsv", "--lineage", "--lineage-clusters", "clusters50.txt"]),
        ("samples and patterns", ["--distances", "distances50.tsv", "--print-samples", "--print-filtered", "--output-patterns", None])]


@pytest.mark.parametrize("tag,extra", RUNS, ids=[r[0] for r in RUNS])
def test_cli_native_and_python_readers_are_byte_identical(tag, extra, tmp_path):
    runs = []
    for reader in ([], ["--python-reader"]):
        pat = str(tmp_path / ("patterns%d.txt" % len(runs)))
        args = PRES + [pat if x is None else x for x in extra]
        pat_name = "patterns%d.txt" % len(runs)
        if tag == "lineage":                                              # (stderr names the file: the same one for both runs)
            args += ["--lineage-file", str(tmp_path / "lineage.txt")]
        out, err = _cli(args + reader)
        written = open(pat, "rb").read() if None in extra else (open(str(tmp_path / "lineage.txt"), "rb").read() if tag == "lineage" else b"")
        runs.append((out, err.replace(pat_name, "patterns.txt"), written))
    assert runs[0] == runs[1]
    assert len(runs[0][0].splitlines()) > 50 and (None not in extra or len(runs[0][2]) > 0)


@pytest.fixture(scope="module")
def default_run():
    return _cli_marked(PRES + ["--distances", "distances50.tsv"])


def test_default_run_takes_the_native_route(default_run):
    out, err, launches = default_run
    assert int(launches) > 0 and len(out.splitlines()) > 50


def test_gpus_keeps_the_line_reader(default_run):
    out, err, launches = _cli_marked(PRES + ["--distances", "distances50.tsv", "--gpus", "0,0"])     # two contexts; the reader is bound to one
    assert launches == "None" and out == default_run[0]


def test_similarity_readers_agree():
    samples = os.path.join(CLI, "samples50.txt")
    a = _cli([samples, "--pres", "kmers120.Rtab", "--min-af", "0.1", "--max-af", "0.8"], module="pyseer_amd.similarity")
    b = _cli([samples, "--pres", "kmers120.Rtab", "--min-af", "0.1", "--max-af", "0.8", "--python-reader"], module="pyseer_amd.similarity")
    assert a == b and len(a[0].splitlines()) == 51


@pytest.mark.parametrize("case", ["rtab_missing_binary", "rtab_missing_continuous"])
def test_predict_readers_agree(case):
    args = [os.path.join(PREDICT, case + ".model"), "samples50.txt", "--pres", os.path.join(ENET, "missing.Rtab")]
    a = _cli(args, module="pyseer_amd.enet_predict")
    b = _cli(args + ["--python-reader"], module="pyseer_amd.enet_predict")
    assert a == b and len(a[0].splitlines()) == 51


def test_predict_looks_only_at_the_lines_the_model_names(tmp_path):
    lines = open(os.path.join(ENET, "missing.Rtab")).read().splitlines()
    bad = "BADROW\t" + "\t".join(["1"] * (len(lines[0].split("\t")) - 2) + ["7"])
    table = str(tmp_path / "bad.Rtab")
    open(table, "w").write("\n".join(lines[:3] + [bad, "ANOTHER\t1", ""] + lines[3:]) + "\n")
    model = open(os.path.join(PREDICT, "rtab_missing_binary.model")).read()
    naming = str(tmp_path / "naming.model")
    open(naming, "w").write(model + "BADROW\t0.3\t0.5\n")
    plain = [os.path.join(PREDICT, "rtab_missing_binary.model"), "samples50.txt"]
    want = _cli(plain + ["--pres", os.path.join(ENET, "missing.Rtab")], module="pyseer_amd.enet_predict")
    for reader in ([], ["--python-reader"]):
        assert _cli(plain + ["--pres", table] + reader, module="pyseer_amd.enet_predict") == want        # the malformed lines are not the model's
        out, err = _cli([naming, "samples50.txt", "--pres", table] + reader, module="pyseer_amd.enet_predict", expect=1)
        assert out == "" and err.endswith("ValueError: Rtab file not binary\n")


# ---- 3. the call blocks into the whole-genome loader -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ref_missing_binary", "ref_missing_continuous"])
def test_call_blocks_load_the_references_rows(name):
    import io
    from pyseer_amd.engine import Engine
    from pyseer_amd.enet import correlation_cut, load_all_vars_calls
    from pyseer_amd.input import iter_call_blocks_rtab_native
    g = np.load(os.path.join(ENET, name + ".npz"))
    p = pd.Series(g["y"], index=[str(s) for s in g["samples"]])
    e = Engine(len(p))
    try:
        blocks = iter_call_blocks_rtab_native(p, os.path.join(ENET, "missing.Rtab"), e, 37)
        M, var_indices, loaded, kept = load_all_vars_calls(e, p, blocks, float(g["min_af"]), float(g["max_af"]), float(g["max_missing"]), io.StringIO())
        assert loaded == int(g["loaded"]) and (np.array(var_indices) == g["var_indices"]).all()
        assert (M.get_rows(np.arange(M.rows)) == g["rows"]).all()
        cor = M.correlations(g["y"])
        for q, key in ((0.25, "kept25"), (0.5, "kept50")):
            assert (correlation_cut(cor, q) == g[key]).all()
        M.close()
    finally:
        e.close()
