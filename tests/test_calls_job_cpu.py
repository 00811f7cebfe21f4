"""--device-calls (SEERHIP_ROUTE calls_job=1) without a device: the plan rules of the route, and the float64 md5 restatement that
tests/test_calls_job_gpu.py holds k_job_md5_calls to, against input.hash_pattern itself."""
import numpy as np
import pytest

from _calls_ref import f64_pattern
from test_cli_run_cpu import plan

VCF = ["--phenotypes", "p.tsv", "--vcf", "v.vcf.gz"]
PRES = ["--phenotypes", "p.tsv", "--pres", "r.Rtab"]


@pytest.mark.parametrize("base", [VCF, PRES, VCF + ["--burden", "regions.txt"]])
def test_the_flag_and_the_route_key_put_call_blocks_on_the_job_stream(base):
    for argv, routes in ((base + ["--device-calls"], {}), (base, {"calls_job": "1"})):
        pl = plan(argv, routes)
        assert pl.job_path and pl.calls_job and not pl.native and not pl.packed_c_loop and not pl.proc_mode
        assert pl.native_vcf == ("--vcf" in base) and pl.native_rtab == ("--pres" in base)
        assert pl.job_block == 1 << 14 and not pl.want_pat                    # bounded blocks; patterns and their count are the stream's
    # blocks end at --block_size where the output depends on block ends
    assert plan(base + ["--device-calls", "--print-filtered"]).job_block == 3000
    assert plan(base + ["--device-calls", "--lmm", "--lineage", "--block_size", "37"]).job_block == 37
    assert plan(base + ["--device-calls", "--block_size", "100000"]).job_block == 100000
    assert plan(base + ["--device-calls", "--output-patterns", "pat.txt"]).want_pat


@pytest.mark.parametrize("base", [VCF, PRES])
def test_what_turns_the_route_off_again(base):
    for extra, routes in ((["--python-sink"], {}), (["--serial-sink"], {}), ([], {"job": "0"}), (["--python-reader"], {})):
        for argv, r2 in ((base + ["--device-calls"] + extra, routes), (base + extra, dict(routes, calls_job="1"))):
            pl = plan(argv, r2)
            assert not pl.job_path and not pl.calls_job, (argv, r2)
            assert pl.job_block == 3000
    pl = plan(PRES + ["--device-calls", "--gpus", "0,0"])                      # (--gpus keeps the line reader for an Rtab, as before)
    assert not pl.job_path and not pl.calls_job and not pl.native_rtab


@pytest.mark.parametrize("base", [VCF, PRES])
def test_without_the_flag_both_inputs_stay_where_they_were(base):
    pl = plan(base)
    assert not pl.job_path and not pl.calls_job and pl.job_block == 3000
    assert not plan(base, {"calls_job": "0"}).calls_job
    # and k-mer input does not know the flag's route
    pk = plan(["--phenotypes", "p.tsv", "--kmers", "k.gz", "--device-calls"])
    assert pk.job_path and not pk.calls_job and pk.job_block == 1 << 18


@pytest.mark.parametrize("N", [15, 63, 64, 65])
def test_float64_md5_restatement_equals_hash_pattern(N):
    from pyseer_amd.input import hash_pattern
    rng = np.random.default_rng(N)
    for trial in range(6):
        p = (rng.random(N) < 0.5).astype(np.uint8)
        m = (rng.random(N) < (0.1, 0.5, 1.0)[trial % 3]).astype(np.uint8)
        if trial == 0:
            m[:] = 0; m[N - 1] = 1                                             # one missing call, the last sample
        k = p.astype(np.float64)
        k[m.astype(bool)] = np.nan                                            # (a missing call wins over a present one: _vcf_packed_block)
        assert f64_pattern(p, m) == hash_pattern(k), (N, trial)
    # a vector without NaN is hashed as int64 by the reference: the two dtypes never give the same digest
    assert f64_pattern(p, np.zeros(N, np.uint8)) != hash_pattern(p.astype(np.int64))
