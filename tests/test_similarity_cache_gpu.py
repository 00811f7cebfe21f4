"""Kinship from a packed cache: `similarity --load-packed` against the reference's own output and against the text route, the rows' one-way
path (sh_sim_accumulate_select: staged, selected and accumulated on the device) against the oracle, and the matrix as text made on the
device (sh_sim_text: k_sim_text_len, k_sim_format) against pandas."""
import ctypes as C
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
pytestmark = pytest.mark.gpu
CLI = os.path.join(os.path.dirname(__file__), "golden", "cli")
SAMPLES = [s.rstrip() for s in open(os.path.join(CLI, "samples50.txt"))]
KMERS = os.path.join(CLI, "kmers.gz")


def _list(path, names):
    with open(path, "w") as f:
        f.write("".join(n + "\n" for n in names))
    return str(path)


def _pack(tmp_path, names, tag):
    from pyseer_amd import pack
    cache = str(tmp_path / (tag + ".seerpack"))
    pack.main([_list(tmp_path / (tag + ".txt"), names), "--kmers", KMERS, "-o", cache])
    return cache


def _run_cli(argv, capsys):
    from pyseer_amd import similarity
    capsys.readouterr()
    similarity.main(argv)
    return capsys.readouterr()


# ---- 1. the cache of the golden k-mer file over its own sample list: the reference's own output ------------------------------------------
def test_cache_over_the_runs_list_prints_the_references_output(tmp_path, capsys):
    cache = _pack(tmp_path, SAMPLES, "own")
    got = _run_cli([os.path.join(CLI, "samples50.txt"), "--load-packed", cache], capsys)
    assert got.out == open(os.path.join(CLI, "expected", "similarity_kmers.tsv")).read()
    assert got.err.splitlines() == open(os.path.join(CLI, "expected", "similarity_kmers.err")).read().splitlines()


# ---- 2. another order, and a superset: stdout is the text route's for the same list and bounds ----------------------------------------------
@pytest.fixture(scope="module")
def run37(tmp_path_factory):
    rng = np.random.default_rng(37)
    d = tmp_path_factory.mktemp("simcache")
    shuffled = [SAMPLES[i] for i in rng.permutation(50)]
    extra = shuffled[:20] + ["nobody_1", "stranger-2"] + shuffled[20:] + ["zz_last"]          # names that no line of the file carries
    run = [SAMPLES[i] for i in rng.permutation(50)[:37]]
    return {"shuffled": _pack(d, shuffled, "shuffled"), "superset": _pack(d, extra, "superset"), "list": _list(d / "run37.txt", run)}


@pytest.mark.parametrize("bounds", [[], ["--min-af", "0.1", "--max-af", "0.8"]], ids=["default_af", "af_0.1_0.8"])
@pytest.mark.parametrize("which", ["shuffled", "superset"])
def test_subset_in_another_order_prints_what_the_text_route_prints(run37, which, bounds, capsys):
    want = _run_cli([run37["list"], "--kmers", KMERS] + bounds, capsys)
    got = _run_cli([run37["list"], "--load-packed", run37[which]] + bounds, capsys)
    assert got.out == want.out
    assert len(got.out.splitlines()) == 38
    said = got.err.splitlines()
    assert said[0] == "pyseer_amd: packed cache holds %d samples; the run's 37 are selected on the device" % (50 if which == "shuffled" else 53)
    assert [l for l in said[1:] if not l.startswith("No observations of ")] == ["Reading in variants", "Matrix size 1000", "Calculating sample similarity"]


# ---- 3. sh_sim_accumulate_select against the oracle --------------------------------------------------------------------------------------
def _source_rows(rng, V, n_src):
    """V x n_src carriers at mixed frequencies, packed at the source width with every padding bit set"""
    from pyseer_amd.packing import pack_variants, row_bytes_for
    rb = row_bytes_for(n_src)
    Kv = (rng.random((V, n_src)) < rng.uniform(0.0, 1.0, V)[:, None]).astype(np.uint8)
    Kv[0] = 1
    padded = np.ones((V, rb * 8), dtype=np.uint8)
    padded[:, :n_src] = Kv
    bits = pack_variants(padded)
    assert bits.shape == (V, rb)
    return Kv, bits


@pytest.mark.parametrize("n_dst", [1, 63, 64, 65, None])
@pytest.mark.parametrize("n_src", [65, 129, 200])
def test_accumulate_select_matches_oracle(n_src, n_dst):
    from oracle import oracle
    from pyseer_amd.engine import Engine, RowSelector
    n_dst = n_src if n_dst is None else n_dst
    rng = np.random.default_rng(1000 * n_src + n_dst)
    sample_map = rng.permutation(n_src)[:n_dst].astype(np.int32)
    e = Engine(n_dst)
    sel = RowSelector(e, n_src, sample_map)
    for V in (1, 64, 65, 1000):
        Kv, bits = _source_rows(rng, V, n_src)
        for lo, hi in ((0.0, 1.0), (0.1, 0.8)):
            e.set_af_filter(lo, hi)
            e.sim_begin()
            sel.sim_accumulate(bits[:V // 2]); sel.sim_accumulate(bits[V // 2:])
            assert np.array_equal(e.sim_finish(), oracle.similarity(Kv[:, sample_map], lo, hi)), (V, lo, hi)
    sel.close(); e.close()


def test_accumulate_select_reuses_its_two_slots():
    """one call stages 128 MB of source rows at a time through two slots: 410 200 rows of 656 bytes are three chunks, the last ragged, so the
    first slot is staged, uploaded and selected a second time while its first rows may still be accumulating"""
    from oracle import oracle
    from pyseer_amd.engine import Engine, RowSelector
    from pyseer_amd.packing import row_bytes_for
    n_src, n_dst = 5200, 64
    rb = row_bytes_for(n_src)
    V = 2 * ((128 << 20) // rb) + 1000
    rng = np.random.default_rng(5200)
    sample_map = rng.permutation(n_src)[:n_dst].astype(np.int32)
    bits = rng.integers(0, 256, size=(V, rb), dtype=np.uint8)
    bits[V // 3:V // 2] &= rng.integers(0, 256, size=(V // 2 - V // 3, rb), dtype=np.uint8)          # (some rarer carriers: the filter drops rows)
    Kv = (bits[:, sample_map >> 3] >> (sample_map & 7).astype(np.uint8)) & 1
    e = Engine(n_dst)
    sel = RowSelector(e, n_src, sample_map)
    e.set_af_filter(0.3, 0.6)
    e.sim_begin()
    sel.sim_accumulate(bits)
    assert np.array_equal(e.sim_finish(), oracle.similarity(Kv, 0.3, 0.6))
    sel.close(); e.close()


def test_accumulate_select_refuses_what_it_cannot_take():
    from pyseer_amd import _abi
    from pyseer_amd.engine import Engine, RowSelector
    e, other = Engine(64), Engine(64)
    sel = RowSelector(e, 129, np.arange(64, dtype=np.int32))
    rows = np.zeros((4, 24), dtype=np.uint8)
    with pytest.raises(_abi.SeerHipError, match="sh_sim_begin has not run"):
        sel.sim_accumulate(rows)
    other.sim_begin()
    rc = e._lib.sh_sim_accumulate_select(other._h, sel._h, rows.ctypes.data_as(_abi.c_u8p), 24, 4)
    assert rc == _abi.SH_EINVAL and b"another context" in e._lib.sh_last_error()
    e.sim_begin()
    with pytest.raises(AssertionError):
        sel.sim_accumulate(np.zeros((4, 16), dtype=np.uint8))                 # 128 bits do not hold 129 samples
    sel.close(); e.close(); other.close()


# ---- 4. sh_sim_text against pandas ----------------------------------------------------------------------------------------------------------
EDGES = [0, 9, 10, 99, 100, 999999, 1000000, 2 ** 31, 10 ** 15 - 1]


def _names(rng, n):
    """lengths 1 to 40 bytes; every third name holds a 2-byte UTF-8 character"""
    out = []
    for j in range(n):
        ln = 1 + (j * 7) % 40 if j else 40
        s = "".join(rng.choice(list("abcXYZ019_.-#|")) for _ in range(ln))
        if j % 3 == 1 and ln >= 2:
            s = s[:ln - 2] + "é"
        assert len(s.encode()) == ln
        out.append(s)
    return out


def _matrix(rng, n):
    K = rng.integers(0, 10 ** 7, size=(n, n)).astype(np.float64)
    at = rng.permutation(n * n)[:min(n * n, 4 * len(EDGES))]
    K.reshape(-1)[at] = [float(EDGES[i % len(EDGES)]) for i in range(at.shape[0])]
    K.reshape(-1)[rng.integers(0, n * n)] = float(EDGES[-1])
    return K


def _pandas_bytes(K, names, mask=None):
    import pandas as pd
    K = np.array(K, dtype=np.float64)
    if mask is not None:
        K[mask, :] = np.nan; K[:, mask] = np.nan
    s = io.StringIO()
    pd.DataFrame(K, index=names, columns=names).to_csv(s, sep='\t')
    return s.getvalue().encode()


def _raw_text(e, K, names, cap, fill=0xAA):
    """sh_sim_text itself -> (rc, *len, the caller's buffer of max(cap, 0) bytes, filled with `fill` beforehand; None for out == NULL)"""
    from pyseer_amd import _abi
    enc = [s.encode() for s in names]
    off = np.zeros(len(enc) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in enc], out=off[1:])
    K = np.ascontiguousarray(K, dtype=np.float64)
    out = None if cap is None else np.full(max(cap, 1), fill, dtype=np.uint8)
    ln = C.c_int64(-1)
    rc = e._lib.sh_sim_text(e._h, K.ctypes.data_as(_abi.c_dp), b"".join(enc), off.ctypes.data_as(C.POINTER(C.c_int64)), None,
                            None if out is None else out.ctypes.data_as(_abi.c_u8p), 0 if cap is None else cap, C.byref(ln))
    return rc, ln.value, out


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129])
def test_sim_text_matches_pandas(n):
    from pyseer_amd import _abi
    from pyseer_amd.engine import Engine
    rng = np.random.default_rng(n)
    names, K = _names(rng, n), _matrix(rng, n)
    e = Engine(n)
    want = _pandas_bytes(K, names)
    assert e.sim_text(names, K=K).tobytes() == want
    one, last, every = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool), np.ones(n, dtype=bool)
    one[n // 3] = True; last[n - 1] = True
    for mask in (np.zeros(n, dtype=bool), one, last, every):
        assert e.sim_text(names, nan_mask=mask, K=K).tobytes() == _pandas_bytes(K, names, mask)
        Kn = K.copy(); Kn[mask, :] = np.nan; Kn[:, mask] = np.nan            # as SimilarityAccumulator.finish hands it on
        assert e.sim_text(names, nan_mask=mask, K=Kn).tobytes() == _pandas_bytes(K, names, mask)
    # the length query, a capacity one byte short (nothing is written), the exact capacity
    rc, ln, _ = _raw_text(e, K, names, None)
    assert (rc, ln) == (_abi.SH_OK, len(want))
    rc, ln, out = _raw_text(e, K, names, len(want) - 1)
    assert (rc, ln) == (_abi.SH_OK, len(want)) and (out == 0xAA).all()
    rc, ln, out = _raw_text(e, K, names, len(want))
    assert (rc, ln) == (_abi.SH_OK, len(want)) and out.tobytes() == want
    # what the notation cannot express is refused, and by name
    for bad, said in ((0.5, "non-integer"), (-1.0, "negative"), (1e15, "1e15 or more")):
        Kb = K.copy(); Kb[n - 1, n // 2] = bad
        with pytest.raises(_abi.SeerHipError, match=said) as ex:
            e.sim_text(names, K=Kb)
        assert ex.value.code == _abi.SH_EINVAL
    with pytest.raises(_abi.SeerHipError, match="tab"):
        e.sim_text(["a\tb"] + names[1:], K=K)
    e.close()


@pytest.mark.parametrize("n_src,n_dst", [(200, 129), (65, 1), (129, 64)])
def test_sim_text_of_the_accumulated_matrix(n_src, n_dst):
    """K = None after an accumulation through the selector: the text of sim_finish()'s matrix"""
    from pyseer_amd.engine import Engine, RowSelector
    rng = np.random.default_rng(n_src + n_dst)
    sample_map = rng.permutation(n_src)[:n_dst].astype(np.int32)
    e = Engine(n_dst)
    sel = RowSelector(e, n_src, sample_map)
    _, bits = _source_rows(rng, 1000, n_src)
    e.sim_begin()
    sel.sim_accumulate(bits[:500]); sel.sim_accumulate(bits[500:])
    names = _names(rng, n_dst)
    K = e.sim_finish()
    assert K.max() >= 100
    text = e.sim_text(names).tobytes()
    assert text == e.sim_text(names, K=K).tobytes() == _pandas_bytes(K, names)
    sel.close(); e.close()
