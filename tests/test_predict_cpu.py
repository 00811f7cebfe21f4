"""The parts of enet_predict that need no device: the model file (enet.write_model / read_model, text and the reference's pickle through a
restricted unpickler), the library's name set (sh_nameset_*) against a Python dict, and the command line's argument errors."""
import collections
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "golden", "cli")


def _bits(x):
    return np.array([x], dtype=np.float64).view(np.uint64)[0]


def test_model_text_round_trip_is_bit_exact(tmp_path):
    from pyseer_amd.enet import read_model, write_model
    rng = np.random.default_rng(3)
    model = collections.OrderedDict()
    model["intercept"] = (1, -0.0)
    model["group 1 hypothetical protein"] = (5e-324, -2.2250738585072014e-308)         # a name with spaces, as Rtab gene names can have
    model["subnormal"] = (2.225073858507201e-308, 4.9406564584124654e-324)
    model["seventeen"] = (0.10000000000000002, -1.2345678901234567e+300)
    model["third"] = (1.0 / 3.0, 2.0 / 3.0)
    for i in range(200):
        model["k%d" % i] = (float(rng.random()), float(rng.normal() * 10.0 ** rng.integers(-300, 300)))
    for continuous in (False, True):
        path = str(tmp_path / ("m%d.txt" % continuous))
        write_model(path, model, continuous)
        back, kind = read_model(path)
        assert kind is continuous and isinstance(back, collections.OrderedDict)
        assert list(back) == list(model)
        for k in model:
            assert _bits(back[k][0]) == _bits(model[k][0]) and _bits(back[k][1]) == _bits(model[k][1]), k
    assert np.signbit(back["intercept"][1])
    with open(path) as fh:
        first = fh.readline().rstrip("\n").split("\t")
    assert first[1] == "version=1" and first[2] == "continuous=1"
    with pytest.raises(ValueError):
        write_model(path, {"a\tb": (0.5, 1.0)}, True)


def test_model_text_refuses_what_it_cannot_read(tmp_path):
    from pyseer_amd.enet import read_model
    for i, text in enumerate(["", "not a model\n", "#pyseer_amd-enet-model\tversion=2\tcontinuous=0\n",
                              "#pyseer_amd-enet-model\tversion=1\tcontinuous=0\nname\t0.5\n", "#pyseer_amd-enet-model\tversion=1\tcontinuous=0\nname\t0.5\tx\n"]):
        path = str(tmp_path / ("bad%d" % i))
        with open(path, "w") as fh:
            fh.write(text)
        with pytest.raises(ValueError):
            read_model(path)


def test_restricted_unpickler(tmp_path):
    from pyseer_amd.enet import read_model
    plain = {"intercept": (1, -0.25), "AAC": (0.25, 1.5), "gene 7": (0.75, -3.0)}
    path = str(tmp_path / "m.pkl")
    for conv in (float, np.float64):
        for protocol in (2, 3, 4, pickle.HIGHEST_PROTOCOL):
            with open(path, "wb") as fh:
                pickle.dump([{k: (conv(a), conv(b)) for k, (a, b) in plain.items()}, False], fh, protocol=protocol)
            model, continuous = read_model(path)
            assert continuous is False and list(model.items()) == [(k, (float(a), float(b))) for k, (a, b) in plain.items()]
            assert all(type(v[0]) is float and type(v[1]) is float for v in model.values())
    ran = str(tmp_path / "ran")

    class Evil(object):
        def __reduce__(self):
            return (os.system, ("touch " + ran,))
    for payload in ([{"a": (0.5, Evil())}, False], [{"a": (0.5, 1.0)}, Evil()], Evil()):
        with open(path, "wb") as fh:
            pickle.dump(payload, fh)
        with pytest.raises(ValueError) as e:
            read_model(path)
        assert "refused" in str(e.value)
        assert not os.path.exists(ran)
    with open(path, "wb") as fh:
        pickle.dump({"a": 1}, fh)                                     # a pickle of only admitted things that is not a model
    with pytest.raises(ValueError):
        read_model(path)


def _blob(names):
    enc = [x.encode() for x in names]
    off = np.zeros(len(enc) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in enc], out=off[1:])
    return b"".join(enc), off


def test_nameset_is_a_dict_that_pops():
    from pyseer_amd.enet import NameSet
    rng = np.random.default_rng(9)
    alphabet = np.array(list("ACGT"))
    pool = ["".join(alphabet[rng.integers(0, 4, size=int(rng.integers(1, 60)))]) for _ in range(150000)]
    pool += [pool[i][:max(1, len(pool[i]) // 2)] for i in range(0, 20000)]        # names that are prefixes of other names
    pool += ["A", "AA", "AAA", "AAAAAAAA", "AAAAAAAAA", "group 1", "group 10"]
    pool = list(dict.fromkeys(pool))
    in_model = [pool[i] for i in rng.choice(len(pool), size=100000, replace=False)]
    ns = NameSet(in_model)
    left = {name: i for i, name in enumerate(in_model)}
    assert ns.left == len(left)
    rows, which = ns.match(b"", np.zeros(1, dtype=np.int64))                        # an empty block
    assert rows.size == 0 and which.size == 0 and ns.left == len(left)
    stream = [pool[i] for i in rng.integers(0, len(pool), size=400000)] + in_model   # duplicates; then every name once more, so all are met
    at = 0
    while at < len(stream):
        block = stream[at:at + int(rng.integers(0, 70000))]
        at += len(block)
        blob, off = _blob(block)
        rows, which = ns.match(blob if at % 2 else np.frombuffer(blob, dtype=np.uint8), off)
        want_rows, want_which = [], []
        for v, name in enumerate(block):
            i = left.pop(name, None)                                                # the reference pops a name when it meets it
            if i is not None:
                want_rows.append(v); want_which.append(i)
        assert rows.tolist() == want_rows and which.tolist() == want_which
        assert ns.left == len(left)
    assert ns.left == 0
    rows, which = ns.match(*_blob(in_model[:100]))
    assert rows.size == 0
    ns.close()
    empty = NameSet([])
    assert empty.left == 0 and empty.match(*_blob(["A"]))[0].size == 0


def _predict(args):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT
    r = subprocess.run([sys.executable, "-m", "pyseer_amd.enet_predict"] + args, cwd=CLI, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    return r.returncode, r.stdout.decode(), r.stderr.decode()


def test_argument_errors(tmp_path):
    model = os.path.join(ROOT, "tests", "golden", "predict", "kmers_binary.model")
    rc, out, err = _predict([model, "samples50.txt"])
    assert rc == 2 and out == "" and "--kmers --vcf --pres" in err
    rc, out, err = _predict([model, "samples50.txt", "--kmers", "kmers.gz", "--pres", "kmers120.Rtab"])
    assert rc == 2 and "not allowed with" in err
    rc, out, err = _predict([model, "samples50.txt", "--kmers", "kmers.gz", "--burden", "regions.txt"])
    assert rc == 1 and out == "" and err == "Burden test can only be performed with VCF input\n"
    rc, out, err = _predict([model, "samples50.txt", "--vcf", "x.vcf.gz", "--load-packed", "x.seerpack"])
    assert rc == 1 and out == "" and err == ("--gpus and the packed cache (--save-packed / --load-packed / --packed-cache / --packed-part) are not "
                                             "available with --vcf\n")
    bad = str(tmp_path / "bad.model")
    with open(bad, "w") as fh:
        fh.write("variant\taf\tbeta\n")
    rc, out, err = _predict([bad, "samples50.txt", "--kmers", "kmers.gz"])
    assert rc == 1 and out == "" and err.startswith("Cannot read the model " + bad)
    rc, out, err = _predict([str(tmp_path / "absent.model"), "samples50.txt", "--kmers", "kmers.gz"])
    assert rc == 1 and out == "" and err.startswith("Cannot read the model ")
    with open(bad, "wb") as fh:
        pickle.dump([{"a": (0.5, os.getcwd)}, False], fh)
    rc, out, err = _predict([bad, "samples50.txt", "--kmers", "kmers.gz"])
    assert rc == 1 and out == "" and "refused" in err


def test_save_model_stays_refused_and_names_the_new_option():
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT
    r = subprocess.run([sys.executable, "-m", "pyseer_amd", "--kmers", "kmers.gz", "--phenotypes", "subset.pheno", "--wg", "enet", "--save-model", "x"],
                       cwd=CLI, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    err = r.stderr.decode()
    assert r.returncode == 1 and "--save-model" in err and "--save-enet-model" in err
