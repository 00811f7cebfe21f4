"""`python -m pyseer_amd` -- pyseer's command line for the per-variant association tests, driving the HIP engine.

Mirrors pyseer/__main__.py for the options that reach the hot path: k-mer / Rtab / VCF input (--vcf, with --burden regions), fixed effects (SEER) with MDS of
a distance matrix or --no-distances, --lmm with a similarity matrix or --load-lmm cache, covariates, continuous
phenotypes, the AF / missing / p-value filters, --print-samples / --print-filtered / --output-patterns, and the four
end-of-run counters.  Variants are parsed in blocks of --block_size, packed, and tested block-wise on the GPU; rows are
printed in the reference's order (fixed effects: input order; LMM: within a block the filtered variants first, then the
tested ones -- fit_lmm returns them that way, lmm.py:160-224).

--lineage (MDS components or --lineage-clusters) runs fit_lineage_effect on the GPU as well (1 + lineages + covariates <= 50; --lineage-clusters
without covariates: up to 1023 clusters).

K-mer text goes through the native reader (csrc/reader.cpp), whose parser reads the sample tokens on the host; --device-reader (one file, one
device) has them read on the device instead (k_kmer_pack), same bytes out; every other route ignores the flag.  --device-inflate implies it and
has the members of a BGZF file decoded on the device too (k_bgzf_inflate); for any other container it is --device-reader.

VCF is read as text (plain, gzip or BGZF; no index, no pysam): natively with the sample columns tokenised on the device, or by the Python
reader (--python-reader).  An Rtab (--pres) goes the same two ways: framed natively with its calls tokenised on the device (k_rtab_pack), or
line by line (--python-reader; also with --gpus, and for a header that names a sample twice).  --device-calls sends the blocks of both native readers to the job
stream as parsed (sh_job_submit_calls: the filters, the rows with missing calls and their patterns on the device, no Python per variant; same bytes out).  --wg enet (pyseer_amd/enet.py run_cli) reads k-mers and VCF, burden regions included, through the native readers
and --pres and --python-reader line by line.  BCF 2.1 / 2.2 is read through --vcf wherever VCF text is (sniffed from the decoded bytes, whatever the file is called): natively with each
record's GT vector reduced on the device (k_bcf_gt_pack), or by the Python reader (--python-reader, input.BcfFile).
--save-calls FILE writes what the native VCF / BCF / Rtab readers deliver -- names, skip reasons, messages, the present and missing planes -- as a call
cache beside the run's usual output; --load-calls FILE reads such a cache (or one written by python -m pyseer_amd.pack over all isolates) instead of a
text file, through the job stream: over the run's own sample list as stored, over a superset or another order of it with both planes restricted to the
run's samples on the device on their way in (k_calls_select, sh_job_submit_calls_select); same bytes out as the text.
Not supported (out of scope): --wg rf / blup, --gpus / the packed k-mer cache with a VCF or BCF, --wg / several devices from a call cache, and around BCF: .csi / .tbi indexes (burden
regions stay one pass over the file), INFO and FORMAT fields other than GT, BCF1 and minor versions above 2 (refused by name), writing BCF.
"""
import argparse
import os
import sys
import time
import warnings

from . import _route


def _torch_reachable(argv):
    """torch is used by the command line for one thing: the eigendecomposition of a similarity matrix on the GPU (--lmm without
    --load-lmm / --cpu-eigh; lmm.spectral_decomposition).  Judged on the raw arguments (argparse accepts unique prefixes), because the
    device warm-up starts before the options are parsed; main() sets the same flag from the parsed options."""
    return any(a.startswith("--lm") for a in argv) and not any(a.startswith("--load-l") or a.startswith("--cpu-e") for a in argv)


def _first_device(argv):
    """The device the run will use first, from the raw arguments: `--gpu N`, `--gpu=N`, `--gpus a,b,...` / `--gpus=a,b` (first listed) or
    `--gpus N` (a count: device 0).  Anything unreadable warms device 0 -- a context on a device the run does not use is the cost."""
    dev = 0
    for i, a in enumerate(argv):
        key, _, val = a.partition("=")
        if key not in ("--gpu", "--gpus"):
            continue
        if not val and i + 1 < len(argv):
            val = argv[i + 1]
        try:
            if key == "--gpu":
                dev = int(val)
            else:
                dev = (_route.device_list(val) or [0])[0]
        except ValueError:
            pass
    return dev


def _warm_device():
    """sh_warmup on a side thread: the HIP runtime's start (0.8 s at N = 5000's first context) runs while the interpreter imports
    numpy / pandas and the inputs are read.  Errors are left to the engine, which reports a missing library or device itself."""
    try:
        dev = _first_device(sys.argv)
        import ctypes
        from . import _abi
        # ctypes.CDLL() holds the GIL through dlopen (the HIP runtime and its dependencies: 0.4 s); dlopen called as a foreign function
        # does not, and makes the CDLL() that follows a look-up
        if not _abi.TORCH_FIRST:                           # (with torch in play its libraries must be loaded first: _abi.load does that)
            libc = ctypes.CDLL(None)
            libc.dlopen.restype = ctypes.c_void_p
            libc.dlopen.argtypes = [ctypes.c_char_p, ctypes.c_int]
            libc.dlopen(_abi.LIB_PATH.encode(), os.RTLD_NOW)
        lib = _abi.load()
        # a job's host threads wait for the device asleep (include/seerhip.h sh_set_wait_mode): the runtime's default spins a CPU per waiting stream
        lib.sh_set_wait_mode(0 if _route.route("wait") == "spin" else 1)
        lib.sh_warmup(dev)
    except Exception:
        pass


_warm_thread = None
if __name__ == "__main__" and "--help" not in sys.argv and "-h" not in sys.argv:
    import atexit
    import threading
    from . import _abi as _abi0
    # written once, on this thread, before the warm-up thread exists and before anyone loads the library; main() reads it back and, should
    # the parsed options disagree with this reading of the raw arguments, decomposes on the CPU rather than import torch after libseerhip
    _abi0.TORCH_FIRST = _torch_reachable(sys.argv)
    _warm_thread = threading.Thread(target=_warm_device, daemon=True)
    _warm_thread.start()
    atexit.register(_warm_thread.join, 10.0)               # an early exit (bad options) must not tear the process down under a running dlopen

from . import __version__, _abi
from .cli_run import (RunContext, die as _die, has_fd, load_inputs, model_state, make_plan, open_blocks, prepare_input,
                      print_header, report_cli, run, setup_engine, validate_loaded, validate_options, write_counters)
from .engine import Engine, PatternSet
from .input import plan_packed_cache
from .lmm import initialise_lmm


def get_options(argv=None):
    description = 'SEER (doi: 10.1038/ncomms12797), reimplemented in python -- MI355X engine (pyseer_amd)'
    parser = argparse.ArgumentParser(description=description, prog="pyseer_amd")
    ph = parser.add_argument_group('Phenotype')
    ph.add_argument('--phenotypes', required=True, help='Phenotypes file (whitespace separated)')
    ph.add_argument('--phenotype-column', default=None, help='Phenotype file column to use [Default: last column]')
    va = parser.add_argument_group('Variants')
    vg = va.add_mutually_exclusive_group(required=True)
    vg.add_argument('--kmers', default=None, nargs='+',
                    help='Kmers file; several files are tested as one stream in the order given and read concurrently (one gzip stream inflates serially)')
    vg.add_argument('--vcf', default=None, help='VCF file. Will filter any non \'PASS\' sites')
    vg.add_argument('--pres', default=None, help='Presence/absence .Rtab matrix as produced by roary and piggy')
    vg.add_argument('--load-calls', default=None, metavar='FILE',
                    help='Read variants from a call cache written by --save-calls or python -m pyseer_amd.pack (--vcf / --pres) instead of parsing the '
                         'VCF, BCF or Rtab again; the cache may hold more samples than the run, in any order (its calls are then selected on the device)')
    va.add_argument('--burden', help='VCF regions to group variants by for burden testing (requires --vcf). '
                    'The regions are assigned in one pass over the file: no index is needed or read')
    di = parser.add_argument_group('Distances')
    dg = di.add_mutually_exclusive_group()
    dg.add_argument('--distances', help='Strains distance square matrix (fixed or lineage effects)')
    dg.add_argument('--load-m', help='Load an existing matrix decomposition')
    sg = di.add_mutually_exclusive_group()
    sg.add_argument('--similarity', help='Strains similarity square matrix (for --lmm)')
    sg.add_argument('--load-lmm', help='Load an existing lmm cache')
    di.add_argument('--save-m', help='Prefix for saving matrix decomposition')
    di.add_argument('--save-lmm', help='Prefix for saving LMM cache')
    di.add_argument('--mds', default="classic", help='Type of multidimensional scaling [Default: classic]')
    di.add_argument('--max-dimensions', type=int, default=10, help='Maximum number of dimensions to consider after MDS')
    di.add_argument('--no-distances', action='store_true', default=False, help='Allow run without a distance matrix')
    asc = parser.add_argument_group('Association options')
    asc.add_argument('--continuous', action='store_true', default=False, help='Force continuous phenotype')
    asc.add_argument('--lmm', action='store_true', default=False, help='Use random instead of fixed effects')
    asc.add_argument('--wg', default=None, help='Use a whole genome model for association and prediction: enet (rf and blup are not built)')
    asc.add_argument('--lineage', action='store_true', help='Report lineage effects')
    asc.add_argument('--lineage-clusters', help='Custom clusters to use as lineages [Default: MDS components]')
    asc.add_argument('--lineage-file', default="lineage_effects.txt", help='File to write lineage association to')
    wg = parser.add_argument_group('Whole genome options')
    wg.add_argument('--sequence-reweighting', action='store_true', help='Use --lineage-clusters to downweight sequences.')
    wg.add_argument('--save-vars', help='(not built: pickles of the reference)')
    wg.add_argument('--load-vars', help='(not built: pickles of the reference)')
    wg.add_argument('--save-model', help='(not built: pickles of the reference; --save-enet-model writes the model as text)')
    wg.add_argument('--save-enet-model', default=None, help='File to save the fitted elastic net to, as text, for python -m pyseer_amd.enet_predict '
                                                            '[Default: do not save the model]')
    wg.add_argument('--save-predictions', default=None, help='File to save predictions to in TSV format [Default: do not save predictions]')
    wg.add_argument('--alpha', type=float, default=0.0069, help='Set the mixing between l1 and l2 penalties [Default: 0.0069]')
    wg.add_argument('--n-folds', type=int, default=10, help='Number of folds cross-validation to perform [Default: 10]')
    wg.add_argument('--enet-seed', type=int, default=1, help='Seed of the random fold assignment (numpy.random.default_rng) [Default: 1]')
    wg.add_argument('--enet-thresh', type=float, default=1e-7, help="Convergence threshold of the coordinate descent (glmnet's thresh) [Default: 1e-7]")
    fi = parser.add_argument_group('Filtering options')
    fi.add_argument('--cor-filter', type=float, default=0.25, help='Correlation filter for elastic net (phenotype/variant correlation quantile at which to start keeping variants) [Default: 0.25]')
    fi.add_argument('--min-af', type=float, default=0.01, help='Minimum AF [Default: 0.01]')
    fi.add_argument('--max-af', type=float, default=0.99, help='Maximum AF [Default: 0.99]')
    fi.add_argument('--max-missing', type=float, default=0.05, help='Maximum missing (vcf/Rtab) [Default: 0.05]')
    fi.add_argument('--filter-pvalue', type=float, default=1, help='Prefiltering t-test pvalue threshold [Default: 1]')
    fi.add_argument('--lrt-pvalue', type=float, default=1, help='Likelihood ratio test pvalue threshold [Default: 1]')
    co = parser.add_argument_group('Covariates')
    co.add_argument('--covariates', default=None, help='User-defined covariates file')
    co.add_argument('--use-covariates', default=None, nargs='*', help="Covariates to use; 'q' suffix = quantitative")
    ot = parser.add_argument_group('Other')
    ot.add_argument('--print-samples', action='store_true', default=False, help='Print sample lists [Default: hide]')
    ot.add_argument('--print-filtered', action='store_true', default=False, help='Print filtered variants [Default: hide]')
    ot.add_argument('--output-patterns', default=False, help='File to print patterns to, useful for finding pvalue threshold')
    ot.add_argument('--count-patterns', default=None, metavar='FILE',
                    help='Count the distinct presence patterns of the tested variants on the GPU while the run goes and write the count and the '
                         'Bonferroni threshold to FILE, as scripts/count_patterns.py prints them for an --output-patterns file')
    ot.add_argument('--pattern-alpha', type=float, default=0.05, help='Family-wise error rate of the --count-patterns threshold [Default: 0.05]')
    ot.add_argument('--uncompressed', action='store_true', default=False, help='Uncompressed kmers file [Default: gzipped]')
    ot.add_argument('--cpu', type=int, default=1, help='Accepted for compatibility; the tests run on the GPU')
    ot.add_argument('--block_size', type=int, default=3000, help='Number of variants parsed and sent to the GPU at a time')
    ot.add_argument('--gpu', type=int, default=0, help='GPU index [Default: 0]')
    ot.add_argument('--gpus', default=None, help='Comma-separated GPU indices, or a count N (= 0..N-1): the variant stream is sharded across them. '
                    'From a packed cache every GPU tests its own contiguous range of the rows through its own pipeline; other input is one stream '
                    'whose blocks go to the GPUs in turn. Output keeps the input order [Default: the single --gpu]')
    ot.add_argument('--save-packed', default=None,
                    help='Also write the parsed k-mer file as packed bit rows (for --load-packed in later runs over the same samples, or any subset or order of them)')
    ot.add_argument('--packed-cache', action='store_true', default=False,
                    help='Keep a packed cache next to the k-mer file (<kmers>.seerpack): written by the first run, read by later runs '
                         'over the same samples while the k-mer file is unchanged (size and modification time); ignored with a warning otherwise')
    ot.add_argument('--load-packed', default=None,
                    help='Read variants from a packed cache written by --save-packed or python -m pyseer_amd.pack instead of parsing --kmers again; the cache may '
                         'hold more samples than the run, in any order (its rows are then selected on one device)')
    ot.add_argument('--save-calls', default=None, metavar='FILE',
                    help='With --vcf (text or BCF, also with --burden) or --pres through the native readers: also write the parsed calls, missing ones '
                         'included, as a call cache in stored blocks of --block_size variants (for --load-calls in later runs over the same samples, or '
                         'any subset or order of them)')
    ot.add_argument('--cpu-eigh', action='store_true', default=False,
                    help='Decompose the similarity matrix with numpy on the host instead of rocSOLVER on the GPU')
    ot.add_argument('--no-dedup', action='store_true', default=False,
                    help='Test every variant separately [Default: each distinct presence pattern of a block is tested once]')
    ot.add_argument('--python-reader', action='store_true', default=False,
                    help='Parse k-mer, VCF and Rtab files with the Python reader instead of the native one')
    ot.add_argument('--device-reader', action='store_true', default=False,
                    help='Read the sample tokens of one --kmers file on the device (the native reader; containers, lines and names stay on the host); '
                         'ignored where another reader is used')
    ot.add_argument('--device-inflate', action='store_true', default=False,
                    help='Decode the members of a BGZF (bgzip) --kmers file on the device as well; implies --device-reader and is ignored where '
                         'that is ignored; for any other container it is --device-reader')
    ot.add_argument('--device-calls', action='store_true', default=False,
                    help='Send the blocks of the native VCF / BCF reader (also with --burden) and of the native Rtab reader to the job stream as '
                         'parsed: the filters, the rows with missing calls and their patterns are handled on the device, and no Python runs per '
                         'variant; same output. Ignored with --python-reader, --python-sink, --serial-sink and --gpus')
    ot.add_argument('--python-sink', action='store_true', default=False,
                    help='Format every output row in Python (one result tuple per variant) instead of the native block sink')
    ot.add_argument('--serial-sink', action='store_true', default=False,
                    help='Format and write each block before the next one is tested [Default: on a worker thread, while the next block is on the GPU]')
    ot.add_argument('--packed-part', default=None, metavar='I/N',
                    help='With --load-packed: run only range I of N contiguous ranges of the cache (one process per device: run N processes, '
                         'each with its own --gpu, and concatenate their outputs in order)')
    ot.add_argument('--lmm-lineage-per-variant', action='store_true', default=False,
                    help='With --lmm --lineage, fit the lineage effect of each variant itself. [Default: reproduce the reference, '
                         'which fits the LAST variant of each block for every variant of that block]')
    ot.add_argument('--version', action='version', version='%(prog)s ' + __version__)
    return parser.parse_args(argv)


def main(argv=None):
    # ---- parse, validate, load the inputs
    options = get_options(argv)
    if __name__ == "__main__":                             # as a program (a caller of main() keeps the library's default: torch first)
        if bool(options.lmm and not options.load_lmm and not options.cpu_eigh) and not _abi.TORCH_FIRST:
            # (the raw-argument reading missed that this run decomposes a kinship matrix: libseerhip may already be loaded without torch's
            # HIP runtime underneath it, and importing torch now would break the device for both)
            sys.stderr.write("pyseer_amd: kinship decomposition on the CPU (numpy) for this run\n")
            options.cpu_eigh = True
    validate_options(options)
    warnings.filterwarnings('ignore')
    inp = load_inputs(options)
    lineage_dict = inp.lineage_dict if options.lineage else None
    if options.wg:
        from . import enet as _enet
        if _warm_thread is not None:
            _warm_thread.join()
        try:
            counts = _enet.run_cli(options, inp.p, inp.cov, inp.m, inp.null_fit, inp.firth_null, inp.lineage_clusters, lineage_dict, inp.clusters_full,
                                   inp.dict_full, inp.enet_seer, sys.stdout, sys.stderr)
        except ValueError as ex_:
            _die(str(ex_) + "\n")
        return write_counters(*counts)

    # ---- set up the model: the kinship cache, then one context per device unless every device gets a process of its own
    t_inputs = time.time()
    plan = make_plan(options, _route.route, has_fd(sys.stdout))
    lmm_fit = None
    if options.lmm:
        sys.stderr.write("Setting up LMM\n")
        # lineage_samples = p.index as the reference passes it (__main__.py:403, 455-456): a similarity matrix over another set of
        # samples is refused here, before p is cut down to it and the lineage design goes out of step with the phenotype
        inp.p, lmm, h2 = initialise_lmm(inp.p, inp.cov, options.similarity, options.load_lmm, options.save_lmm,
                                        lineage_samples=(inp.p.index if options.lineage else None), use_gpu=not options.cpu_eigh, device=options.gpu)
        sys.stderr.write("h^2 = " + '{0:.2f}'.format(h2) + "\n")
        lmm_fit = (lmm, h2)
    p = inp.p
    state = model_state(options, inp, lmm_fit, (options.min_af, options.max_af) if (plan.native or options.load_packed or plan.calls_job) else None)
    engs = []
    if not plan.proc_mode:
        # One context per listed device; the same device may be listed twice (two contexts on one GPU: the test of
        # the multi-device job path on a one-GPU box)
        if _warm_thread is not None:
            _warm_thread.join()                            # (the device's wait mode is chosen at its first use: by the warm-up, not by a context racing it)
        _abi.load().sh_set_wait_mode(0 if _route.route("wait") == "spin" else 1)
        engs = [Engine(len(p), device=d) for d in ([options.gpu] if plan.devices is None else plan.devices)]
        for e_ in engs:
            setup_engine(e_, state, share_from=(engs[0] if e_ is not engs[0] else None))
    t_setup = time.time()

    # ---- plan: what needs the run's samples, the files behind the header line, the route of the blocks
    cache_selected = validate_loaded(options, plan, p)
    src = prepare_input(options, plan, p)
    patterns = open(options.output_patterns, 'wb') if options.output_patterns else None
    print_header(options, inp.cov)
    cache_stamp = None
    if options.packed_cache and plan.native and not options.load_packed and not options.save_packed:
        cache_stamp = plan_packed_cache(options, p, src.var_file)
    plan = make_plan(options, _route.route, has_fd(sys.stdout), patterns is None or has_fd(patterns), cache_selected,
                     engs[0].get_lanes() if engs else None, proc_mode=plan.proc_mode)
    ctx = RunContext(state, options, p, p.values.astype(float), 'lmm' if options.lmm else 'seer', lineage_dict, plan, engs, patterns=patterns)
    if options.count_patterns:
        ctx.count_set = PatternSet(engs[0])

    # ---- run, report
    try:
        prefilter, tested, printed = run(ctx, open_blocks(ctx, src, cache_stamp))
    except BaseException:
        if src.calls_out is not None:                      # (--save-calls: a run that fails leaves no cache)
            src.calls_out.abort()
        raise
    if src.calls_out is not None:
        src.calls_out.close()
    if src.selector is not None:
        src.selector.close()
    if _route.debug("cli"):
        report_cli(ctx, t_inputs, t_setup)
    if patterns is not None:
        patterns.close()
    if ctx.count_set is not None:
        from .count_patterns import result_text
        n_patterns = ctx.count_set.count()
        ctx.count_set.close()
        with open(options.count_patterns, 'w') as fh:
            fh.write(result_text(n_patterns, options.pattern_alpha))
    if src.cache_out is not None:
        src.cache_out.close()
    for e_ in engs:
        e_.close()
    write_counters(prefilter, tested, printed)


if __name__ == "__main__":
    main()
