"""pyseer_amd/cli_run.py without a device: the --gpus helper, the plan of a run on a table of its rules, and the state that the devices'
processes are set up from, written and read back."""
from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest

from pyseer_amd import _route
from pyseer_amd.__main__ import _first_device, get_options
from pyseer_amd.cli_run import make_plan, model_state, read_state, write_state

K = ["--phenotypes", "p.tsv", "--kmers", "k.gz"]
R = ["--phenotypes", "p.tsv", "--pres", "r.Rtab"]
C = ["--load-packed", "c.seerpack"]
G2 = ["--gpus", "0,0"]


@pytest.mark.parametrize("gpus,devices", [(None, None), ("3", [0, 1, 2]), ("0,0,0", [0, 0, 0]), ("2,5", [2, 5]), ("1", [0]), ("7,", None)])
def test_device_list_and_the_warm_up_agree(gpus, devices):
    if gpus == "7,":                                                    # unreadable: the run stops there, the warm-up falls back to device 0
        with pytest.raises(ValueError):
            _route.device_list(gpus)
        assert _first_device(["prog", "--gpus", gpus]) == 0
        return
    assert _route.device_list(gpus) == devices
    if gpus is not None:
        assert _first_device(["prog", "--gpus", gpus]) == _first_device(["prog", "--gpus=" + gpus]) == devices[0]
    assert _first_device(["prog", "--gpu", "4"]) == 4 and _first_device(["prog"]) == 0


def test_device_count_counts_an_unreadable_list_by_its_entries():
    """--count-patterns has always refused `--gpus 7,` for its two entries; a single unreadable value stops the run as it did"""
    assert [_route.device_count(g) for g in (None, "1", "3", "0,0", "7,", "a,b,c")] == [0, 1, 3, 2, 2, 3]
    with pytest.raises(ValueError):
        _route.device_count("x")


def plan(argv, routes=None, **facts):
    """the plan as main() makes it behind the header line: stdout and the pattern file have descriptors, three lanes, unless told otherwise"""
    facts = dict(dict(stdout_fd=True, patterns_fd=True, cache_selected=False, lanes=3), **facts)
    return make_plan(get_options(argv), lambda key, default=None: (routes or {}).get(key, default), **facts)


# (argv, routes, facts) -> the fields named; every rule as the command line has always applied it
TABLE = [
    # job_block: block_size with --print-filtered, with the reference's LMM lineage, or outside the job stream; else at least 2^18
    (K, {}, {}, dict(job_path=True, job_block=1 << 18, job_ahead=5, native=True, lmm_block_lineage=False)),
    (K + ["--block_size", "500000"], {}, {}, dict(job_block=500000)),
    (K + ["--print-filtered"], {}, {}, dict(job_path=True, job_block=3000)),
    (K + ["--lmm", "--lineage"], {}, {}, dict(job_path=True, lmm_block_lineage=True, job_block=3000, job_ahead=2)),
    (K + ["--lmm", "--lineage", "--lmm-lineage-per-variant"], {}, {}, dict(lmm_block_lineage=False, job_block=1 << 18)),
    (K + ["--lineage"], {}, {}, dict(lmm_block_lineage=False, job_block=1 << 18)),
    (K + ["--python-sink", "--block_size", "77"], {}, {}, dict(job_path=False, job_block=77, job_ahead=2)),
    (K, {}, dict(lanes=None), dict(job_path=True, job_ahead=2)),
    # job_path: off for either sink option, for job=0, for input that is neither native k-mers nor a cache
    (K + ["--serial-sink"], {}, {}, dict(job_path=False, job_block=3000)),
    (K, {"job": "0"}, {}, dict(job_path=False, job_block=3000)),
    (K, {"job": "py"}, {}, dict(job_path=True, packed_c_loop=False)),
    (K + ["--python-reader"], {}, {}, dict(native=False, job_path=False)),
    (R, {}, {}, dict(var_type="Rtab", native=False, native_rtab=True, job_path=False, job_block=3000)),
    (R + C, {}, {}, dict(native_rtab=False, job_path=True, packed_c_loop=True)),
    (["--phenotypes", "p.tsv", "--vcf", "v.vcf"], {}, {}, dict(var_type="vcf", native_vcf=True, native=False, job_path=False)),
    (["--phenotypes", "p.tsv", "--vcf", "v.vcf", "--python-reader"], {}, {}, dict(native_vcf=False)),
    # packed_c_loop: a cache through the job stream, unless job=py, a selected cache, or no descriptor to write to
    (K + C, {}, {}, dict(job_path=True, packed_c_loop=True, cache_selected=False, proc_mode=False)),
    (K + C, {"job": "py"}, {}, dict(packed_c_loop=False)),
    (K + C, {"job": "0"}, {}, dict(packed_c_loop=False)),
    (K + C, {}, dict(cache_selected=True), dict(packed_c_loop=False, cache_selected=True, job_path=True)),
    (K + C, {}, dict(stdout_fd=False), dict(packed_c_loop=False)),
    (K + C, {}, dict(patterns_fd=False), dict(packed_c_loop=False)),
    (K, {}, {}, dict(packed_c_loop=False)),
    # proc_mode: more than one device and --load-packed, and nothing that keeps the streams in this process
    (K + C + G2, {}, {}, dict(devices=[0, 0], proc_mode=True, packed_c_loop=True)),
    (K + C + ["--gpus", "2"], {}, {}, dict(devices=[0, 1], proc_mode=True)),
    (K + C + ["--gpus", "1"], {}, {}, dict(devices=[0], proc_mode=False)),
    (K + C, {}, {}, dict(devices=None, proc_mode=False)),
    (K + G2, {}, {}, dict(proc_mode=False)),
    (K + C + G2 + ["--save-packed", "d.seerpack"], {}, {}, dict(proc_mode=False)),
    (K + C + G2 + ["--python-sink"], {}, {}, dict(proc_mode=False)),
    (K + C + G2 + ["--serial-sink"], {}, {}, dict(proc_mode=False)),
    (K + C + G2 + ["--packed-part", "0/2"], {}, {}, dict(proc_mode=False)),
    (K + C + G2, {"job": "0"}, {}, dict(proc_mode=False)),
    (K + C + G2, {"job": "py"}, {}, dict(proc_mode=False)),
    (K + C + G2, {"procs": "0"}, {}, dict(proc_mode=False, packed_c_loop=True)),
    (K + C + G2, {}, dict(stdout_fd=False), dict(proc_mode=False)),
    (K + C + G2, {}, dict(proc_mode=False), dict(proc_mode=False)),           # (decided before the contexts were made: it stands)
    # native_rtab: off with --gpus or any packed-cache option
    (R + ["--gpus", "1"], {}, {}, dict(native_rtab=False)),
    (R + ["--save-packed", "d.seerpack"], {}, {}, dict(native_rtab=False)),
    (R + ["--packed-cache"], {}, {}, dict(native_rtab=False)),
    (R + ["--packed-part", "0/2"], {}, {}, dict(native_rtab=False)),
    (R + ["--python-reader"], {}, {}, dict(native_rtab=False)),
    # the device reader: off with --gpus, implied by --device-inflate; the two route keys
    (K, {}, {}, dict(dev_reader=False, dev_inflate=False)),
    (K + ["--device-reader"], {}, {}, dict(dev_reader=True, dev_inflate=False)),
    (K + ["--device-inflate"], {}, {}, dict(dev_reader=True, dev_inflate=True)),
    (K + ["--device-reader", "--gpus", "1"], {}, {}, dict(dev_reader=False)),
    (K + ["--device-inflate", "--gpus", "1"], {}, {}, dict(dev_reader=False, dev_inflate=True)),
    (K, {"kmer_dev": "1"}, {}, dict(dev_reader=True, dev_inflate=False)),
    (K, {"kmer_inflate": "1"}, {}, dict(dev_reader=True, dev_inflate=True)),
    # want_pat: --output-patterns, or --count-patterns outside the job stream
    (K, {}, {}, dict(want_pat=False)),
    (K + ["--output-patterns", "pat.txt"], {}, {}, dict(want_pat=True)),
    (K + ["--count-patterns", "n.txt"], {}, {}, dict(job_path=True, want_pat=False)),
    (K + ["--count-patterns", "n.txt", "--python-sink"], {}, {}, dict(job_path=False, want_pat=True)),
    (K + ["--count-patterns", "n.txt"], {"job": "0"}, {}, dict(want_pat=True)),
]


@pytest.mark.parametrize("argv,routes,facts,want", TABLE, ids=["%02d" % i for i in range(len(TABLE))])
def test_plan_rules(argv, routes, facts, want):
    got = plan(argv, routes, **facts)._asdict()
    assert {k: got[k] for k in want} == want


def test_plan_before_the_contexts_decides_proc_mode_from_the_options_as_given():
    """main() plans once before a context exists, from stdout's descriptor alone: what it needs then are the devices, proc_mode and the readers."""
    early = make_plan(get_options(K + C + G2), _route.route, True)
    assert early.proc_mode and early.devices == [0, 0] and early.native and not early.native_rtab
    assert not make_plan(get_options(K + C + G2), _route.route, False).proc_mode


def _same(a, b):
    assert sorted(a) == sorted(b)
    for k, v in a.items():
        if isinstance(v, np.ndarray):
            assert isinstance(b[k], np.ndarray) and b[k].dtype == v.dtype and np.array_equal(b[k], v), k
        else:
            assert not isinstance(b[k], np.ndarray) and b[k] == v and type(b[k]) is type(v), k


def test_state_round_trip_lmm_and_fixed_effects(tmp_path):
    rng = np.random.default_rng(3)
    n = 7
    p = pd.Series(rng.integers(0, 2, n).astype(float), index=["s%d" % i for i in range(n)])
    opts = dict(lmm=True, continuous=False, filter_pvalue=0.5, lrt_pvalue=0.01, no_dedup=False, print_filtered=True, lineage=False,
                lmm_lineage_per_variant=False, print_samples=True)
    inp = SimpleNamespace(p=p, cov=pd.DataFrame([]), m=np.empty((0, 0)), null_fit=None, firth_null=True, lineage_clusters=None, lineage_dict=None)
    lmm = SimpleNamespace(U=rng.normal(size=(n, n)), S=rng.random(n), Y=p.values.reshape(-1, 1), X=np.ones((n, 1)))
    st = model_state(SimpleNamespace(**opts), inp, (lmm, np.float64(0.37)), (0.01, 0.99))
    assert st["lmm"] and st["h2"] == 0.37 and st["sample_names"] == list(p.index) and st["lineage_labels"] is None and st["lin"] is None
    full = dict(st, devices=[0, 0], patterns=True, job_block=1 << 18, dma=True, path="/x/c.seerpack")
    d = tmp_path / "lmm"
    d.mkdir()
    write_state(str(d), full)
    _same(full, read_state(str(d)))

    cov = pd.DataFrame(rng.normal(size=(n, 2)), index=p.index, columns=["a", "b"])
    opts.update(lmm=False, lineage=True, print_samples=False, no_dedup=True)
    inp = SimpleNamespace(p=p, cov=cov, m=rng.normal(size=(n, 2)), null_fit=SimpleNamespace(llf=-3.25), firth_null=-2.5,
                          lineage_clusters=rng.integers(0, 2, (n, 3)), lineage_dict=["l1", "l2", "l3"])
    st = model_state(SimpleNamespace(**opts), inp, None, None)
    assert not st["lmm"] and st["W"].shape == (n, 4) and np.array_equal(st["W"][:, 2:], cov.values) and st["llf"] == -3.25 and st["firth_null"] == -2.5
    assert st["lineage_labels"] == ["l1", "l2", "l3"] and st["lin"].dtype == np.float64 and st["lin"].shape == (n, 3) and np.array_equal(st["lin_cov"], cov.values)
    assert st["af_filter"] is None and st["sample_names"] is None and st["no_dedup"] is True
    d = tmp_path / "fixed"
    d.mkdir()
    write_state(str(d), st)
    _same(st, read_state(str(d)))
