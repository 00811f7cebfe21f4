"""The refusals of the command line that need no input file: python -m pyseer_amd called in process as main([...]), each one held to exit status 1
and to the exact text on stderr.  A command line that is wrong twice gets the message of the refusal that comes first."""
import pytest

from pyseer_amd.__main__ import main

K = ["--phenotypes", "p.tsv", "--kmers", "k.gz"]
V = ["--phenotypes", "p.tsv", "--vcf", "v.vcf"]
ND = ["--no-distances"]
VCF_CACHE = "--gpus and the packed cache (--save-packed / --load-packed / --packed-cache / --packed-part) are not available with --vcf\n"
PICKLES = "%s writes pickles of reference-internal objects and is not built in pyseer_amd\n"
STRUCTURE = ("Must use distance matrix with fixed effects, or similarity matrix with random effects\n"
             "Unless performing a lineage analysis with random effects\n")
NO_DISTANCES = "Option --no-distances must be used when no distance matrix is provided\n"

CASES = [
    ("burden without vcf", K + ND + ["--burden", "b.txt"], "Burden test can only be performed with VCF input\n"),
    ("lmm with wg", K + ["--lmm", "--similarity", "s.tsv", "--wg", "enet"], "Choose only one alternative model. Either --lmm, --wg or neither\n"),
    ("wg rf", K + ["--wg", "rf"], "Whole-genome model 'rf' is not built in pyseer_amd (only --wg enet is)\n"),
    ("enet save-vars", K + ["--wg", "enet", "--save-vars", "f"], PICKLES % "--save-vars"),
    ("enet load-vars", K + ["--wg", "enet", "--load-vars", "f"], PICKLES % "--load-vars"),
    ("enet save-model", K + ["--wg", "enet", "--save-model", "f"],
     PICKLES % "--save-model" + "--save-enet-model FILE writes the fitted model as text for python -m pyseer_amd.enet_predict\n"),
    ("enet gpus", K + ["--wg", "enet", "--gpus", "2"], "--wg enet runs on one device: --gpus and --packed-part are not available with it\n"),
    ("vcf gpus", V + ND + ["--gpus", "2"], VCF_CACHE),
    ("vcf save-packed", V + ND + ["--save-packed", "c"], VCF_CACHE),
    ("vcf load-packed", V + ND + ["--load-packed", "c"], VCF_CACHE),
    ("vcf packed-cache", V + ND + ["--packed-cache"], VCF_CACHE),
    ("vcf packed-part", V + ND + ["--packed-part", "0/2"], VCF_CACHE),
    ("count-patterns wg", K + ["--wg", "enet", "--count-patterns", "n.txt"], "Whole genome model does not produce patterns. Re-run without --count-patterns.\n"),
    ("count-patterns two devices", K + ND + ["--count-patterns", "n.txt", "--gpus", "0,0"],
     "--count-patterns counts on one device: it is not available with more than one device in --gpus\n"),
    ("count-patterns a count of two", K + ND + ["--count-patterns", "n.txt", "--gpus", "2"],
     "--count-patterns counts on one device: it is not available with more than one device in --gpus\n"),
    ("count-patterns an unreadable list of two", K + ND + ["--count-patterns", "n.txt", "--gpus", "7,"],
     "--count-patterns counts on one device: it is not available with more than one device in --gpus\n"),
    ("count-patterns packed-part", K + ND + ["--count-patterns", "n.txt", "--load-packed", "c", "--packed-part", "0/2"],
     "--count-patterns counts one whole run: it is not available with --packed-part\n"),
    # (one device in --gpus is no refusal of --count-patterns: the command line goes on to the next thing wrong with it)
    ("count-patterns one device", K + ["--count-patterns", "n.txt", "--gpus", "1"], NO_DISTANCES),
    ("alpha", K + ["--wg", "enet", "--alpha", "2"], "--alpha must lie in [0, 1]\n"),
    ("max-dimensions", K + ["--distances", "d.tsv", "--max-dimensions", "0"], "Minimum number of dimensions after MDS is 1\n"),
    ("lmm without similarity", K + ["--lmm"], "Must provide a similarity matrix or lmm cache for random effects\n"),
    ("lmm with distances", K + ["--lmm", "--similarity", "s.tsv", "--distances", "d.tsv"], STRUCTURE),
    ("fixed with similarity", K + ["--distances", "d.tsv", "--similarity", "s.tsv"], STRUCTURE),
    ("lmm lineage without distances", K + ["--lmm", "--similarity", "s.tsv", "--lineage"], "Must also provide a distance matrix to report lineage effects\n"),
    ("fixed without distances", K, NO_DISTANCES),
    ("no-distances with distances", K + ND + ["--distances", "d.tsv"], "Cannot use --no-distances with --distances or --load-m\n"),
    ("no-distances with load-m", K + ND + ["--load-m", "m.pkl"], "Cannot use --no-distances with --distances or --load-m\n"),
    ("no-distances lineage without clusters", K + ND + ["--lineage"],
     "Must provide a lineage clusters file when --no-distances and --lineage are used together in fixed-effects mode\n"),
    ("no-distances lmm", K + ND + ["--lmm", "--similarity", "s.tsv"], "Cannot use --no-distances with --lmm\n"),
    ("reweighting without clusters", K + ["--wg", "enet", "--sequence-reweighting"],
     "Using sequence reweighting requires clusters to weight with.\nProvide these with --lineage-clusters. Incompatible with --lineage.\n"),
    ("reweighting with lineage", K + ["--wg", "enet", "--sequence-reweighting", "--lineage-clusters", "c.txt", "--lineage"],
     "Using sequence reweighting requires clusters to weight with.\nProvide these with --lineage-clusters. Incompatible with --lineage.\n"),
    ("wg output-patterns", K + ["--wg", "enet", "--output-patterns", "pat.txt"], "Whole genome model does not produce patterns.\nRe-run without --output-patterns.\n"),
    ("block_size", K + ND + ["--block_size", "0"], "Block size must be at least 1\n"),
    # wrong twice and more: the first refusal answers
    ("order: burden first", K + ["--burden", "b.txt", "--lmm", "--wg", "enet", "--block_size", "0"], "Burden test can only be performed with VCF input\n"),
    ("order: vcf before the model", V + ["--gpus", "2", "--lmm", "--wg", "enet", "--block_size", "0"], VCF_CACHE),
    ("order: model before block_size", K + ["--lmm", "--wg", "enet", "--block_size", "0"], "Choose only one alternative model. Either --lmm, --wg or neither\n"),
    ("order: dimensions before structure", K + ["--max-dimensions", "0", "--block_size", "0"], "Minimum number of dimensions after MDS is 1\n"),
]


@pytest.mark.parametrize("tag,argv,text", CASES, ids=[c[0] for c in CASES])
def test_refusal_exits_1_with_its_message(tag, argv, text, capsys):
    with pytest.raises(SystemExit) as ex:
        main(argv)
    assert ex.value.code == 1
    got = capsys.readouterr()
    assert got.err == text and got.out == ""
