"""Goldens of python -m pyseer_amd.enet_predict, written to tests/golden/predict/ by the reference's own predictor.

    python make_predict_golden.py <checkout of the reference>

Per case: <case>.model (the model as the text of pyseer_amd.enet.write_model -- data: names and numbers; the pickle the reference reads is
made from it on the fly, here and in the tests), <case>.out and <case>.err (what pyseer.enet_predict.main printed), and cases.json (the
arguments).  The reference runs under tests/golden/_harness with the glmnet and pysam stand-ins and, where statsmodels is not installed,
the inert one of _harness/stubs_predict (the predictor never calls it).  It cannot read a VCF here (the pysam stand-in raises) and its
--true-values block does not run on a current numpy; the tests cover those two against other yardsticks.

The models are drawn by a seeded generator over the names of cli/kmers.gz (and enet/missing.Rtab): about 40 names, frequencies on both
sides of 0.5, slopes of both signs, one slope that is exactly 0, one name the input does not hold.  The generator asserts that at least one
drawn line has no carrier among the 50 samples (the draw is repeated until it holds one), so that the reference's "No observations of ..." message is part of the golden."""
import collections
import gzip
import json
import os
import pickle
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "predict")
CLI = os.path.join(HERE, "cli")
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from pyseer_amd.enet import read_model, write_model  # noqa: E402

ABSENT = "GATTACAGATTACAGATTACAGATTACA_not_in_the_input"
KMERS = ["--kmers", "kmers.gz"]
COV = ["--covariates", "covariates.txt", "--use-covariates", "2q", "3"]
RTAB = ["--pres", os.path.join("..", "enet", "missing.Rtab")]


def draw(seed, names, n, intercept=True, covariates=(), need_one_of=()):
    """need_one_of: the draw is repeated (same generator, next values) until it holds one of these names."""
    rng = np.random.default_rng(seed)
    while True:
        model = _draw(rng, names, n, intercept, covariates)
        if not need_one_of or set(model).intersection(need_one_of):
            return model


def _draw(rng, names, n, intercept, covariates):
    model = collections.OrderedDict()
    if intercept:
        model["intercept"] = (1, float(rng.normal()))
    for c in covariates:
        model[c] = (float(rng.uniform(0.5, 3.0)), float(rng.normal(scale=0.3)))
    picked = [names[i] for i in sorted(rng.choice(len(names), size=n, replace=False))]
    order = rng.permutation(n)                             # the model's order is not the input's
    for j, i in enumerate(order):
        af = float(rng.uniform(0.02, 0.98))
        beta = 0.0 if j == 3 else float(rng.normal(scale=0.7))
        model[picked[i]] = (af, beta)
        if j == n // 2:
            model[ABSENT] = (float(rng.uniform(0.02, 0.98)), float(rng.normal(scale=0.7)))
    return model


def main():
    reference = os.path.abspath(sys.argv[1])
    with open(os.path.join(CLI, "samples50.txt")) as fh:
        samples = set(line.rstrip() for line in fh)
    kmer_names, empty = [], []
    with gzip.open(os.path.join(CLI, "kmers.gz"), "rt") as fh:
        for line in fh:
            kmer_names.append(line.split()[0])
            if not samples.intersection(x.split(":")[0] for x in line.rstrip().split("|")[1].split()):
                empty.append(kmer_names[-1])
    with open(os.path.join(HERE, "enet", "missing.Rtab")) as fh:
        rtab_names = [line.split("\t")[0] for line in fh][1:]
    cases = collections.OrderedDict()
    cases["kmers_binary"] = (draw(11, kmer_names, 40, need_one_of=empty), False, KMERS)
    cases["kmers_continuous"] = (draw(12, kmer_names, 40, need_one_of=empty), True, KMERS)
    cases["kmers_cov_binary"] = (draw(13, kmer_names, 40, need_one_of=empty, covariates=("quantitative", "categorical_0", "not_loaded")), False, KMERS + COV)
    cases["kmers_cov_continuous"] = (draw(14, kmer_names, 40, need_one_of=empty, covariates=("quantitative",)), True, KMERS + COV)
    cases["kmers_ignore_missing_binary"] = (draw(11, kmer_names, 40, need_one_of=empty), False, KMERS + ["--ignore-missing"])
    cases["kmers_ignore_missing_continuous"] = (draw(12, kmer_names, 40, need_one_of=empty), True, KMERS + ["--ignore-missing"])
    cases["kmers_threshold"] = (draw(11, kmer_names, 40, need_one_of=empty), False, KMERS + ["--threshold", "0.3"])
    cases["rtab_missing_binary"] = (draw(15, rtab_names, 40), False, RTAB)
    cases["rtab_missing_continuous"] = (draw(16, rtab_names, 40), True, RTAB)
    cases["no_intercept"] = (draw(17, kmer_names, 40, need_one_of=empty, intercept=False), True, KMERS)
    env = dict(os.environ)
    harness = os.path.join(HERE, "_harness")
    env["PYTHONPATH"] = os.pathsep.join([harness, os.path.join(harness, "stubs")] +
                                        ([] if _have("statsmodels") else [os.path.join(harness, "stubs_predict")]) + [reference])
    env["PYTHONDONTWRITEBYTECODE"] = "1"
    os.makedirs(OUT, exist_ok=True)
    listing = collections.OrderedDict()
    for name, (model, continuous, args) in cases.items():
        path = os.path.join(OUT, name + ".model")
        write_model(path, model, continuous)
        back, kind = read_model(path)
        assert kind == continuous and list(back.items()) == [(k, (float(a), float(b))) for k, (a, b) in model.items()]
        with tempfile.TemporaryDirectory() as tmp:
            pkl = os.path.join(tmp, "model.pkl")
            with open(pkl, "wb") as fh:
                pickle.dump([dict(model), continuous], fh)
            r = subprocess.run([sys.executable, "-W", "ignore", os.path.join(harness, "run_enet_predict.py"), pkl, "samples50.txt"] + args, cwd=CLI, env=env,
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0, r.stderr.decode()
        err = r.stderr.decode()
        assert ("Could not find covariate/variant " + ABSENT) in err
        if name.startswith("kmers"):
            assert "No observations of " in err, "no drawn line of %s is without a carrier: choose another seed" % name
        if name.startswith("rtab"):
            assert b"\tnan" in r.stdout
        with open(os.path.join(OUT, name + ".out"), "wb") as fh:
            fh.write(r.stdout)
        with open(os.path.join(OUT, name + ".err"), "wb") as fh:
            fh.write(r.stderr)
        listing[name] = {"args": args, "continuous": continuous}
        print(name, len(r.stdout), "bytes of stdout;", err.count("No observations"), "lines without a carrier;", r.stdout.count(b"nan"), "nan")
    with open(os.path.join(OUT, "cases.json"), "w") as fh:
        json.dump(listing, fh, indent=1)
        fh.write("\n")


def _have(module):
    import importlib.util
    return importlib.util.find_spec(module) is not None


if __name__ == "__main__":
    main()
