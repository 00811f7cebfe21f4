"""fit_lineage_effect (pyseer/model.py:151-199) by the count kernel (k_glm_lineage_counts, csrc/glm_lineage.hip): designs of cluster
indicators without covariates, which need no dense Hessian -- the route a design of more than 49 clusters takes (the dense kernels stop at
1 + lineages + covariates = 50), and SEERHIP_ROUTE lin_counts=1 forces for narrower ones.

Held to oracle.lineage_effect where the oracle reaches (63 columns), to the same engine's dense route where that runs, and beyond both to
the numpy restatement of the reference's arithmetic (tests/_lineage_ref.py: wald_dense; for the cases of YARDSTICK_CASES its values come
from tests/golden/lincounts_dense.npz, l = 1000 takes seconds per row).  The agreement rule (_lineage_ref.check_rows): -1 matches None
exactly; an index g that is not the yardstick's argmax must have wald_dense[g] >= max (1 - DELTA), and at most 10 % of a case's rows may
agree only that way."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lineage_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _engine(monkeypatch, N, lin_counts=None):
    """An engine whose context was created under SEERHIP_ROUTE lin_counts=<value> (None: unset, the default rule)."""
    from pyseer_amd import _route
    from pyseer_amd.engine import Engine
    monkeypatch.setenv("SEERHIP_ROUTE", _route.with_route(os.environ.get("SEERHIP_ROUTE"), lin_counts=lin_counts))
    return Engine(N)


def _fit(monkeypatch, N, lin, K, lin_counts=None, cov=None):
    from pyseer_amd.engine import pack_variants
    e = _engine(monkeypatch, N, lin_counts)
    try:
        e.lineage_setup(lin, cov)
        return e.lineage_batch(pack_variants(K))
    finally:
        e.close()


def _agree(got, want, cluster_of, l, K):
    """got (-1: None) against another implementation's answers `want` (None or index): equal, or agreeing under the rule on wald_dense."""
    lin = R.design(cluster_of, l)
    cnt = [R.counts(cluster_of, l, k) for k in K]
    cond = [R.well_conditioned(*c) for c in cnt]
    dense = []
    for i, (g, w) in enumerate(zip(got, want)):
        if not cond[i] or (w is None and g < 0) or (w is not None and int(g) == w):
            dense.append(None if w is None else (w, np.nan, {}))
            continue
        assert w is not None and g >= 0, "row %d: got %r, want %r" % (i, int(g), w)
        wd = R.wald_dense(lin, K[i])
        assert wd is not None, "row %d: got %r, want %r, the yardstick None" % (i, int(g), w)
        dense.append((int(np.argmax(wd)), float(np.max(wd)), wd))
    return R.check_rows(got, dense, cond, l, cnt=cnt, loose_max=R.loose_bound(cnt, cond, dense))


def test_refusal_lifted(monkeypatch):
    """60 clusters at N = 300: refused before the count kernel ('1 + lineages + covariates must be <= 50'), and still with lin_counts=0 or
    with covariates -- which the message now names."""
    from pyseer_amd._abi import SeerHipError
    N, l, V = 300, 60, 40
    cluster_of, K = R.oracle_case(N, l, V, 7)
    lin = R.design(cluster_of, l)
    got = _fit(monkeypatch, N, lin, K)
    cnt = [R.counts(cluster_of, l, k) for k in K]
    cond, dense = [R.well_conditioned(*c) for c in cnt], R.dense_rows(lin, K)
    R.check_rows(got, dense, cond, l, cnt=cnt, loose_max=R.loose_bound(cnt, cond, dense))
    with pytest.raises(SeerHipError, match="<= 50"):
        _fit(monkeypatch, N, lin, K, lin_counts=0)
    cov = np.random.default_rng(3).standard_normal((N, 2))
    with pytest.raises(SeerHipError, match="this one has covariates"):
        _fit(monkeypatch, N, lin, K, cov=cov)
    mds = lin.copy(); mds[0, 0] = 0.5
    with pytest.raises(SeerHipError, match="not the indicators"):
        _fit(monkeypatch, N, mds, K)


# Rows of test_counts_vs_oracle's cases, by (l, N), on which the DENSE kernels answer None and the oracle fits (never the other way; measured
# on these inputs, every other case 0): a cluster without carriers that has jumped past the ridge's pole leaves h_c ~ 1e-90 on the diagonal,
# and the kernels' factorisations (LDL in registers up to l = 15, LU with pivoting in k_glm_wide_lineage_blk above) round a pivot to an exact
# zero where numpy's and the oracle's do not.  The count kernel agrees with the oracle on every one of these rows.  Known, not fixed here
# (DESIGN.md section 9); the table bounds how many rows the route-against-route comparison may leave out.
DENSE_NONE_ROWS = {(2, 65): 1, (2, 130): 1, (15, 63): 2, (15, 65): 1, (15, 130): 2, (15, 1000): 1, (16, 65): 24, (16, 130): 1,
                   (17, 64): 3, (17, 65): 26, (17, 130): 15, (17, 1000): 3, (49, 65): 223, (49, 130): 252, (49, 1000): 15}


@pytest.mark.parametrize("N", [63, 64, 65, 130, 1000])
@pytest.mark.parametrize("l", [1, 2, 15, 16, 17, 49, 50, 63])
def test_counts_vs_oracle(monkeypatch, l, N):
    """Against oracle.lineage_effect on 257 rows; the route forced where the default is the dense kernels (1 + l <= 50), and there against
    those kernels on the same rows as well."""
    from oracle import oracle as orc
    V = 257
    cluster_of, K = R.oracle_case(N, l, V, 100 * N + l)
    lin = R.design(cluster_of, l)
    got = _fit(monkeypatch, N, lin, K, lin_counts=1 if l + 1 <= 50 else None)
    Kf = K.astype(float)
    first = orc.lineage_effect(lin, None, Kf[0])                             # (loads the oracle before the threads share it)
    with ThreadPoolExecutor(16) as pool:
        want = [first] + list(pool.map(lambda v: orc.lineage_effect(lin, None, Kf[v]), range(1, V)))
    tied, _ = _agree(got, want, cluster_of, l, K)
    print("N %d l %d: %d rows None, %d rows through the tolerance" % (N, l, sum(w is None for w in want), tied))
    if l + 1 <= 50:
        # On all the rows but those where the dense route itself differs from the oracle about None: DENSE_NONE_ROWS, counted and bounded.
        dense = [None if x < 0 else int(x) for x in _fit(monkeypatch, N, lin, K)]
        same = [v for v in range(V) if (dense[v] is None) == (want[v] is None)]
        print("N %d l %d: the dense route differs from the oracle in None on %d rows" % (N, l, V - len(same)))
        assert V - len(same) <= DENSE_NONE_ROWS.get((l, N), 0)
        _agree(got[same], [dense[v] for v in same], cluster_of, l, K[same])


_cases = {}


def _case(N, l, tame):
    if (N, l, tame) not in _cases:
        cluster_of, K = R.yardstick_case(N, l, tame=tame)
        cnt = [R.counts(cluster_of, l, k) for k in K]
        cond = [R.well_conditioned(*c) for c in cnt]
        _cases[(N, l, tame)] = (R.design(cluster_of, l), K, R.fixture_rows(N, l, tame)[0], cond, cnt)
    return _cases[(N, l, tame)]


@pytest.mark.parametrize("tame", [False, True])
@pytest.mark.parametrize("V", [1, 63, 64, 65, 300])
@pytest.mark.parametrize("N,l", R.YARDSTICK_CASES)
def test_counts_vs_yardstick(monkeypatch, N, l, V, tame):
    """Rows with the cluster sizes and carrier rates of _lineage_ref.yardstick_case.  As drawn (tame False), most rows hold a cluster of
    carriers only, on which the reference's answer is rounding noise (_lineage_ref.well_conditioned): of those no more may differ from the
    yardstick than _lineage_ref.loose_bound allows; the rule holds the others.  tame: the same rows with such clusters broken: all but those with a pure reference cluster are held
    by the rule."""
    lin, K, dense, cond, cnt = _case(N, l, tame)
    got = _fit(monkeypatch, N, lin, K[:V])
    tied, loose = R.check_rows(got, dense[:V], cond[:V], l, cnt=cnt[:V], loose_max=R.loose_bound(cnt[:V], cond[:V], dense[:V]))
    print("N %d l %d V %d tame %d: %d rows None, %d well-conditioned, %d of them through the tolerance, %d of the others differ" %
          (N, l, V, tame, sum(d is None for d in dense[:V]), sum(cond[:V]), tied, loose))


@pytest.mark.parametrize("l,lin_counts", [(5, 1), (60, None)])
def test_edge_rows(monkeypatch, l, lin_counts):
    from pyseer_amd.engine import pack_variants
    N = 130
    rng = np.random.default_rng(l)
    cluster_of = np.zeros(N, dtype=np.uint16)
    cluster_of[40:40 + l] = np.arange(1, l + 1)                              # every cluster once, then two or three more of the first ones
    cluster_of[40 + l:] = (np.arange(N - 40 - l) % min(l, 30)) + 1
    lin = R.design(cluster_of, l)
    ref = np.flatnonzero(cluster_of == 0)
    rows, want = [], []

    def add(k, w):
        rows.append(np.asarray(k, dtype=np.uint8)); want.append(w)
    add(np.zeros(N), -1)                                                     # all 0, all 1: PerfectSeparationError
    add(np.ones(N), -1)
    add(cluster_of == 2, -1)                                                 # one cluster's indicator: pure everywhere
    add(np.isin(cluster_of, [0, 1, 3]), -1)                                  # pure in every cluster, the reference's all carriers
    k = np.zeros(N); k[ref[::4]] = 1                                         # mixed in the reference cluster alone
    add(k, "yardstick")
    k = k.copy(); k[np.flatnonzero(cluster_of == 3)[:1]] = 1                 # ... and in cluster 3 alone: its index, 2
    add(k, 2)
    K = np.stack(rows)
    e = _engine(monkeypatch, N, lin_counts)
    try:
        e.lineage_setup(lin)
        bits = pack_variants(K)
        got = e.lineage_batch(bits)
        again = e.lineage_batch(bits)
        dirty = bits.copy()
        if N % 8:
            dirty[:, N // 8] |= np.uint8((0xFF << (N % 8)) & 0xFF)           # the padding bits behind sample N - 1, set
        dirty[:, (N + 7) // 8:] = 0xFF
        got_dirty = e.lineage_batch(dirty)
        empty = lin.copy(); empty[cluster_of == 4, 3] = 0                    # an empty column (its samples join the reference cluster)
        e.lineage_setup(empty)
        got_empty = e.lineage_batch(bits)
    finally:
        e.close()
    assert (got == again).all() and (got == got_dirty).all(), (got, again, got_dirty)
    for i, w in enumerate(want):
        wd = R.wald_dense(lin, K[i])
        if w != "yardstick":
            assert (wd is None) == (w < 0) and (w < 0 or int(np.argmax(wd)) == w), (i, w, wd)   # the yardstick agrees with the hand's answer
            assert got[i] == w, (i, got, w)
    cnt = [R.counts(cluster_of, l, k) for k in K]
    R.check_rows(got, R.dense_rows(lin, K), cnt=cnt)                         # (clusters without carriers tie, far below cluster 3)
    assert (got_empty == -1).all(), got_empty


# ---- the command line ----------------------------------------------------------------------------------------------------------------------
def _write_set(tmp_path):
    """300 samples, 80 clusters (79 columns once the command line has dropped the one least tied to the phenotype: c000, 63 samples at
    the phenotype's overall rate), 400 k-mers (carrier rates per cluster, so that lineages matter), a binary phenotype."""
    rng = np.random.default_rng(11)
    N = 300
    names = ["s%03d" % i for i in range(N)]
    label = np.array([0] * 63 + [1 + i // 3 for i in range(237)])
    y = np.zeros(N, dtype=int)
    y[:63] = np.arange(63) % 2
    for c in range(79):
        y[63 + 3 * c:66 + 3 * c] = [1, 0, 1] if c % 2 else [0, 1, 0]
    y[62] = 1                                                               # (150 of 300: c000 holds 32 of 63, the rate of all)
    perm = rng.permutation(N)
    (tmp_path / "pheno.tsv").write_text("samples\tbinary\n" + "".join("%s\t%d\n" % (names[i], y[i]) for i in perm))
    (tmp_path / "clusters.txt").write_text("".join("%s\tc%03d\n" % (names[i], label[i]) for i in perm))
    K = np.zeros((400, N), dtype=np.uint8)
    for v in range(400):
        rate = np.where(rng.random(80) < 0.5, rng.uniform(0.0, 0.15), rng.uniform(0.3, 0.9, 80))
        K[v] = rng.random(N) < np.clip(rate[label] + 0.25 * (y - 0.5) * (v % 3 == 0), 0, 1)
    R.break_full_clusters(label, 79, K, rng)                                # (every row well conditioned: _lineage_ref.well_conditioned)
    lines = []
    for v in range(400):
        kmer = "".join("ACGT"[(v >> (2 * b)) & 3] for b in range(12)) + "ACGTACGTACGTACGTACGT"
        lines.append(kmer + " | " + " ".join("%s:1" % names[i] for i in np.flatnonzero(K[v])) + "\n")
    import gzip
    with gzip.open(str(tmp_path / "kmers.gz"), "wt") as fh:
        fh.writelines(lines)
    D = (K[:, :, None] != K[:, None, :]).sum(axis=0).astype(float)
    with open(str(tmp_path / "dist.tsv"), "w") as fh:
        fh.write("\t" + "\t".join(names) + "\n")
        for i in range(N):
            fh.write(names[i] + "\t" + "\t".join("%g" % x for x in D[i]) + "\n")
    (tmp_path / "samples.txt").write_text("".join(n + "\n" for n in names))
    return names, label, K, {l.split(" ")[0]: v for v, l in enumerate(lines)}


def _run(args, cwd, route=None):
    env = dict(os.environ); env["PYTHONPATH"] = ROOT
    env.pop("SEERHIP_ROUTE", None)
    if route:
        env["SEERHIP_ROUTE"] = route
    r = subprocess.run([sys.executable, "-m"] + args, cwd=str(cwd), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return r


@pytest.mark.parametrize("model", ["fixed", "lmm"])
def test_cli_eighty_clusters(model, tmp_path):
    """--lineage --lineage-clusters with 80 clusters (79 columns) through the job stream and through --python-sink: the same bytes; the lineage
    column under the agreement rule.  --lmm fits the lineage of a block's last variant for the whole block (LinList mode 2 and the
    one-row call), pyseer/lmm.py:209-213."""
    names, label, K, row_of = _write_set(tmp_path)
    base = ["pyseer_amd", "--kmers", "kmers.gz", "--phenotypes", "pheno.tsv", "--lineage", "--lineage-clusters", "clusters.txt", "--print-filtered"]
    if model == "lmm":
        r = _run(["pyseer_amd.similarity", "--kmers", "kmers.gz", "samples.txt"], tmp_path)
        (tmp_path / "sim.tsv").write_bytes(r.stdout)
        base += ["--lmm", "--similarity", "sim.tsv", "--distances", "dist.tsv", "--block_size", "64"]
    else:
        base += ["--no-distances"]
    outs = []
    for tag, extra in (("job", []), ("sink", ["--python-sink"])):
        r = _run(base + extra + ["--lineage-file", "lin.txt"], tmp_path)
        outs.append((r.stdout, r.stderr, (tmp_path / "lin.txt").read_bytes()))
    assert outs[0] == outs[1]
    dropped = outs[0][2].decode().splitlines()[-1].split("\t")[0]
    assert dropped == "c000"
    cluster_of = label.astype(np.uint16)                                    # c000 is the reference cluster, column a is c%03d of a + 1
    lin = R.design(cluster_of, 79)
    text = outs[0][0].decode().splitlines()
    hdr = text[0].split("\t")
    col, ncol = hdr.index("lineage"), hdr.index("notes")
    rows = [t.split("\t") for t in text[1:]]
    assert len(rows) > 100
    # the rows the reference fits a lineage for (model.py:379-382; lmm.py:200-213: one fit per block of 64 k-mers, its last one's, reported
    # for the block's rows that passed the filters)
    skip = {"af-filter", "pre-filtering-failed"} | ({"lrt-filtering-failed"} if model == "lmm" else {"firth-fail"})
    keep = [f for f in rows if not (set(f[ncol].split(",") if len(f) > ncol else []) & skip)]
    assert len(keep) > 50
    got = [(-1 if f[col] == "NA" else int(f[col][1:]) - 1) for f in keep]
    src = [row_of[f[0]] for f in keep]
    if model == "lmm":
        src = [min(400, (v // 64 + 1) * 64) - 1 for v in src]
    dense = {v: d for v, d in zip(sorted(set(src)), R.dense_rows(lin, K[sorted(set(src))]))}
    cnt = [R.counts(cluster_of, 79, K[v]) for v in src]
    cond = [R.well_conditioned(*c) for c in cnt]
    assert sum(cond) > 0.9 * len(cond)
    dl = [dense[v] for v in src]
    R.check_rows(got, dl, cond, 79, cnt=cnt, loose_max=R.loose_bound(cnt, cond, dl))
    assert any(g >= 0 for g in got)
