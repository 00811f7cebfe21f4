"""The command line behind pyseer_amd/__main__.py main: the refusals, the host set-up, the plan of a run (RunPlan), what its runners share (RunContext), the five
ways a run goes -- one process per device, one thread per device, the library's own loop over a cache, the job stream driven from Python, the Python block loop --
and the SEERHIP_DEBUG=cli report.  A device's process (_packed_child.py) sets up through setup_engine / make_job too: pandas is imported inside the parent's functions only."""
import codecs, collections, ctypes, json, os, pickle, queue, resource, shutil, subprocess, sys, tempfile, threading, time
from types import SimpleNamespace

import numpy as np

from . import _abi, _route
from .classes import Seer, LMM, FLAG_FILTER, FLAG_PREFILTER, notes_from_flags
from .engine import Job
from .lmm import mask_like_fit_lmm
from .model import fit_null, covariate_block, host_pre_filtering
from .packing import pack_variants
from .sink import RowFormatter, names_blob
from .utils import format_output

NOTE_AF, NOTE_FIRTH_FAIL = 1, 1 << 6
_utf8 = codecs.getincrementaldecoder("utf-8")()            # for a caller's stdout that is a text stream without a binary layer: the streams carry bytes


def die(msg):
    sys.stderr.write(msg)
    sys.exit(1)


def has_fd(f):
    try:
        return f.fileno() >= 0
    except Exception:
        return False


def binary_stdout():
    return sys.stdout.buffer if hasattr(sys.stdout, "buffer") else sys.stdout


def write_stdout(b):
    sys.stdout.flush()                                     # (the header line sits in the text layer's buffer)
    out = binary_stdout()
    out.write(b if out is not sys.stdout else _utf8.decode(bytes(b)))     # (incremental: a name may straddle two chunks of join_parts)


def join_parts(parts, write):
    """The per-device parts of an output (binary files), through `write` in the order of the input, behind what part 0 wrote itself."""
    for f in parts:
        f.seek(0)
        for chunk in iter(lambda: f.read(1 << 22), b""):
            write(chunk)
        f.close()


def write_counters(prefilter, tested, printed):
    sys.stderr.write('%d loaded variants\n%d pre-filtered variants\n%d tested variants\n%d printed variants\n' % (prefilter + tested, prefilter, tested, printed))


# ---- the refusals ----------------------------------------------------------------------------------------------------------------------------
def refuse_cache_clashes(options):
    if options.load_packed and options.save_packed and os.path.realpath(options.load_packed) == os.path.realpath(options.save_packed):
        # (the cache is memory-mapped while it is read: rewriting it under the mapping would end the run with SIGBUS)
        die('--save-packed and --load-packed name the same file\n')
    if options.kmers and len(options.kmers) > 1 and (options.python_reader or options.load_packed or options.save_packed or options.packed_cache):
        die('Several --kmers files need the native reader and cannot be combined with a packed cache\n')


def refuse_call_cache_clashes(options):
    """--save-calls and --load-calls against the options they do not go with (a call cache: input.py CallCacheWriter)."""
    kmer_cache = options.save_packed or options.load_packed or options.packed_cache
    if options.save_calls:
        if options.load_calls:
            die('--save-calls writes the calls a VCF, BCF or Rtab is parsed into: not available with --load-calls\n')
        if options.kmers:
            die('--save-calls caches VCF, BCF and Rtab calls: k-mers have --save-packed\n')
        if options.python_reader:
            die('--save-calls writes what the native readers deliver: not available with --python-reader\n')
        if options.gpus is not None:
            die('--save-calls is written by a run on one device: not available with --gpus\n')
        if options.wg:
            die('--save-calls is written by a per-variant run: not available with --wg\n')
        if kmer_cache or options.packed_part:
            die('--save-calls is no packed k-mer cache: not available with --save-packed / --load-packed / --packed-cache / --packed-part\n')
    if options.load_calls:
        if options.burden:
            die('--load-calls serves the variants its cache holds: --burden regions are not applied to it (write the cache with --save-calls --burden)\n')
        if _route.device_count(options.gpus) > 1:
            die('--load-calls selects and tests on one device: not available with more than one device in --gpus\n')
        if options.packed_part:
            die('--load-calls reads one whole cache: not available with --packed-part\n')
        if options.wg:
            die('--load-calls serves the per-variant models: not available with --wg\n')
        if kmer_cache:
            die('--load-calls reads a call cache, not a packed k-mer cache: not available with --save-packed / --load-packed / --packed-cache\n')


def validate_options(options):
    """Every refusal that needs the options alone, in the order a doubly-wrong command line is answered in."""
    refuse_call_cache_clashes(options)
    if options.burden and not options.vcf:
        die('Burden test can only be performed with VCF input\n')
    if options.count_patterns:
        # (the set of distinct patterns lives on one device, in one process: a union across devices or processes is not built)
        if options.wg:
            die("Whole genome model does not produce patterns. Re-run without --count-patterns.\n")
        if _route.device_count(options.gpus) > 1:
            die("--count-patterns counts on one device: it is not available with more than one device in --gpus\n")
        if options.packed_part:
            die("--count-patterns counts one whole run: it is not available with --packed-part\n")
    if options.vcf and (options.gpus is not None or options.save_packed or options.load_packed or options.packed_cache or options.packed_part):
        die('--gpus and the packed cache (--save-packed / --load-packed / --packed-cache / --packed-part) are not available with --vcf\n')
    if options.lmm and options.wg:
        die('Choose only one alternative model. Either --lmm, --wg or neither\n')
    if options.wg and options.wg != 'enet':
        die("Whole-genome model '%s' is not built in pyseer_amd (only --wg enet is)\n" % options.wg)
    if options.wg:
        for name_, val_ in (('--save-vars', options.save_vars), ('--load-vars', options.load_vars), ('--save-model', options.save_model)):
            if val_:
                die('%s writes pickles of reference-internal objects and is not built in pyseer_amd\n' % name_ +
                    ('--save-enet-model FILE writes the fitted model as text for python -m pyseer_amd.enet_predict\n' if name_ == '--save-model' else ''))
        if options.gpus is not None or options.packed_part:
            die('--wg enet runs on one device: --gpus and --packed-part are not available with it\n')
        if (options.load_packed or options.save_packed or options.packed_cache or (options.kmers and len(options.kmers) > 1)) and \
                (options.python_reader or options.pres or not (options.kmers or options.load_packed)):
            # (raw blocks and the cache hold k-mer lines, which have no missing calls: --vcf has its own native route without a cache, --pres and
            # --python-reader keep the line-by-line path)
            die('--wg enet reads one variant file through the Python readers: the packed cache and several --kmers files are not available with it\n')
        refuse_cache_clashes(options)                      # (--python-reader with several files was answered just above)
        if not (0.0 <= options.alpha <= 1.0):
            die('--alpha must lie in [0, 1]\n')
    if options.max_dimensions < 1:
        die('Minimum number of dimensions after MDS is 1\n')
    if options.lmm and not options.similarity and not options.load_lmm:
        die('Must provide a similarity matrix or lmm cache for random effects\n')
    if not options.no_distances:
        if (options.lmm and (options.distances or options.load_m) and not options.lineage) or (not options.lmm and (options.similarity or options.load_lmm)):
            sys.stderr.write('Must use distance matrix with fixed effects, or similarity matrix with random effects\n')
            die('Unless performing a lineage analysis with random effects\n')
        if options.lmm and not (options.distances or options.load_m) and options.lineage:
            die('Must also provide a distance matrix to report lineage effects\n')
        if not options.lmm and not options.wg and not options.distances and not options.load_m:
            die('Option --no-distances must be used when no distance matrix is provided\n')
    else:
        if options.distances or options.load_m:
            die('Cannot use --no-distances with --distances or --load-m\n')
        if not options.lmm and not options.wg and not options.lineage_clusters and options.lineage:
            die('Must provide a lineage clusters file when --no-distances and --lineage are used together in fixed-effects mode\n')
        if options.lmm:
            die('Cannot use --no-distances with --lmm\n')
    if options.wg and options.sequence_reweighting and (not options.lineage_clusters or options.lineage):
        sys.stderr.write("Using sequence reweighting requires clusters to weight with.\n")
        die("Provide these with --lineage-clusters. Incompatible with --lineage.\n")
    if options.wg and options.output_patterns:
        sys.stderr.write("Whole genome model does not produce patterns.\n")
        die("Re-run without --output-patterns.\n")
    if options.block_size < 1:
        die('Block size must be at least 1\n')


def validate_loaded(options, plan, p):
    """The refusals that need the run's samples, once the contexts are set up.  Returns whether --load-packed names a cache over a superset or another order of the run's
    samples (input.py iter_packed_blocks_cached, select): its rows are restricted and permuted on the first device while the cache is read, in the Python block loop of one
    device.  (A cache that cannot be used at all raises where it always has: at the library's header check or at the first block, behind the header line.)"""
    from .input import announce_cache_select
    cache_selected = False
    if options.load_packed:
        try:
            cache_selected = announce_cache_select(p, options.load_packed, select="device")
        except (ValueError, IOError, OSError):
            pass
        if cache_selected and ((plan.devices is not None and len(plan.devices) > 1) or options.packed_part):
            die("pyseer_amd: a packed cache over other samples than the run's own list is read on one device: not with --gpus or --packed-part\n")
    refuse_cache_clashes(options)
    return cache_selected


def call_cache_select_mode():
    """How --load-calls restricts a cache over other samples than the run's own list: "fused" (sh_job_submit_calls_select), "rows" (SEERHIP_ROUTE
    calls_cache=rows: sh_select_calls, then sh_job_submit_calls) or "host" (cache_select=host: the host restatement)."""
    if _route.route("cache_select") == "host":
        return "host"
    return "rows" if _route.route("calls_cache") == "rows" else "fused"


def open_run_call_cache(path, p):
    """--load-calls before the header line: the cache opened, once, with its own checks (a file that is no call cache or is truncated; a run sample it
    lacks; a sample listed twice), each answered in one line, and for a cache over a superset or another order of the run's samples the one line
    that says so.  Returns (stored names, the stored blocks' iterator of open_call_cache, the sample map -- None for the run's own list)."""
    from .input import open_call_cache, call_cache_sample_map
    try:
        stored, _, _, blocks = open_call_cache(path)
        sample_map = call_cache_sample_map(stored, [str(x) for x in p.index])
    except (ValueError, IOError, OSError) as ex:
        die("pyseer_amd: --load-calls: %s\n" % ex)
    if sample_map is not None:
        sys.stderr.write("pyseer_amd: call cache holds %d samples; the run's %d are selected on the %s\n"
                         % (len(stored), len(p), "host" if call_cache_select_mode() == "host" else "device"))
    return stored, blocks, sample_map


# ---- the host set-up ---------------------------------------------------------------------------------------------------------------------------
def load_inputs(options):
    """Phenotypes, covariates, the MDS of the distances with the null fits, the lineage design with its effects file (pyseer/__main__.py:334-444)."""
    import pandas as pd
    from .input import load_phenotypes, load_structure, load_covariates, load_lineage
    p = load_phenotypes(options.phenotypes, options.phenotype_column)
    sys.stderr.write("Read " + str(len(p)) + " phenotypes\n")
    if not options.continuous:
        options.continuous = p.values[(p.values != 0) & (p.values != 1)].size > 0
        sys.stderr.write("Detected %s phenotype\n" % ("continuous" if options.continuous else "binary"))
    cov = load_covariates(options.covariates, options.use_covariates, p) if options.covariates is not None else pd.DataFrame([])
    if cov is None:
        sys.exit(1)
    m = np.empty(shape=(0, 0))
    null_fit = firth_null = None
    enet_seer = bool(options.wg and options.distances or options.load_m)          # pyseer/__main__.py:334-336
    if (options.lineage and not options.lineage_clusters) or enet_seer or not (options.lmm or options.wg):
        if not options.no_distances:
            if options.load_m and os.path.isfile(options.load_m):
                mdf = pd.read_pickle(options.load_m)
                sys.stderr.write("Loaded projection with dimension " + str(mdf.shape) + "\n")
            else:
                seed = os.environ.get('PYSEERSEED', None)
                mdf = load_structure(options.distances, p, options.max_dimensions, options.mds, options.cpu, int(seed) if seed is not None else None)
                if options.save_m:
                    mdf.to_pickle(options.save_m + ".pkl")
            if options.max_dimensions > mdf.shape[1]:
                sys.stderr.write('Population MDS scaling restricted to %d dimensions instead of requested %d\n' % (mdf.shape[1], options.max_dimensions))
                options.max_dimensions = mdf.shape[1]
            inter = p.index.intersection(mdf.index)
            sys.stderr.write("Analysing " + str(len(inter)) + " samples found in both phenotype and structure matrix\n")
            p = p.loc[inter]
            m = mdf.loc[p.index].values[:, :options.max_dimensions]
        if cov.shape[1] > 0:
            cov = cov.loc[p.index]
        null_fit = fit_null(p.values, m, cov, options.continuous)
        firth_null = fit_null(p.values, m, cov, options.continuous, True) if not (options.continuous or options.lmm) else True
        if null_fit is None or firth_null is None:
            die('Could not fit null model, exiting\n')
    # lineage effects (pyseer/__main__.py:388-444)
    lineage_clusters = lineage_dict = None
    if options.lineage_clusters:
        lineage_clusters, lineage_dict = load_lineage(options.lineage_clusters, p)
    clusters_full, dict_full = (np.copy(lineage_clusters), list(lineage_dict)) if options.lineage_clusters else (None, lineage_dict)
    if options.lineage:
        from scipy.stats import norm
        lineage_wald = {}
        if options.lineage_clusters:
            # one-hot clusters are not full rank: drop the cluster least associated with the phenotype
            for lineage, design in zip(lineage_dict, lineage_clusters.T):
                lf = fit_null(p.values, design.reshape(-1, 1).astype(float), cov, options.continuous)
                if lf is None:
                    die('Could not fit lineage null model, exiting\n')
                lineage_wald[lineage] = np.absolute(lf.params[1]) / lf.bse[1]
            min_lineage = min(lineage_wald.items(), key=lambda kv: kv[1])[0]
            drop = lineage_dict.index(min_lineage)
            lineage_clusters = np.delete(lineage_clusters, drop, 1)
            del lineage_dict[drop]
        else:
            lineage_dict = ["MDS" + str(i + 1) for i in range(options.max_dimensions)]
            lineage_clusters = m
            for lineage, slope, se in zip(lineage_dict, null_fit.params[1:], null_fit.bse[1:]):
                lineage_wald[lineage] = np.absolute(slope) / se
        sys.stderr.write('Writing lineage effects to %s\n' % options.lineage_file)
        with open(options.lineage_file, 'w') as lineage_out:
            lineage_out.write("\t".join(["lineage", "wald_test", "p-value"]) + "\n")
            for lineage, wald in sorted(lineage_wald.items(), key=lambda kv: kv[1], reverse=True):
                lineage_out.write("\t".join([lineage, str(wald), str(2 * (1 - norm.cdf(wald)))]) + "\n")
    return SimpleNamespace(p=p, cov=cov, m=m, null_fit=null_fit, firth_null=firth_null, enet_seer=enet_seer, lineage_clusters=lineage_clusters,
                           lineage_dict=lineage_dict, clusters_full=clusters_full, dict_full=dict_full)


def model_state(options, inp, lmm_fit, af_filter):
    """What an engine and a Job are set up from, as plain scalars and arrays: setup_engine and make_job read it in this process, and in every device's process
    behind write_state / read_state.  lmm_fit: (lmm, h2) of initialise_lmm, None for fixed effects; af_filter: the AF window where the device applies it."""
    p, cov = inp.p, inp.cov
    st = {"n": len(p), "lmm": bool(options.lmm), "continuous": bool(options.continuous), "filter_pvalue": options.filter_pvalue, "lrt_pvalue": options.lrt_pvalue,
          "no_dedup": bool(options.no_dedup), "af_filter": af_filter, "print_filtered": bool(options.print_filtered),
          "lineage_labels": (list(inp.lineage_dict) if options.lineage else None), "lineage_per_variant": bool(options.lmm_lineage_per_variant),
          "sample_names": ([str(x) for x in p.index] if options.print_samples else None), "lin": (np.asarray(inp.lineage_clusters, dtype=float) if options.lineage else None),
          "lin_cov": (np.asarray(cov.values, dtype=float) if (options.lineage and cov.shape[1] > 0) else None)}
    if options.lmm:
        lmm, h2 = lmm_fit
        st.update(U=lmm.U, S=lmm.S, Y=lmm.Y, X=lmm.X, h2=float(h2))
    else:
        st.update(y=np.asarray(p.values, dtype=float), W=covariate_block(len(p), inp.m, cov), llf=(float("nan") if options.continuous else float(inp.null_fit.llf)),
                  firth_null=(None if options.continuous else float(inp.firth_null)))
    return st


def write_state(d, state):
    """`state` into directory d for the devices' processes: its arrays as arrays.npz, everything else as state.pkl."""
    arrays = {k: v for k, v in state.items() if isinstance(v, np.ndarray)}
    np.savez(os.path.join(d, "arrays.npz"), **arrays)
    with open(os.path.join(d, "state.pkl"), "wb") as fh:
        pickle.dump({k: v for k, v in state.items() if k not in arrays}, fh)


def read_state(d):
    with open(os.path.join(d, "state.pkl"), "rb") as fh, np.load(os.path.join(d, "arrays.npz")) as a:
        return dict(pickle.load(fh), **{k: a[k] for k in a.files})


def setup_engine(engine, st, share_from=None):
    """The set-up of one context from model_state.  share_from: a context of this process that is set up already -- the LMM's per-run state (M = U~ diag(1/Sd) U~^T,
    limbs, tables) is received from it device to device (sh_lmm_share: 94 MB at N = 5000) instead of re-derived from the host copy of U."""
    if st["lmm"] and share_from is not None:
        engine.lmm_share_from(share_from)
    elif st["lmm"]:
        engine.lmm_setup(st["U"], st["S"], st["Y"], st["X"], st["h2"], st["continuous"], st["filter_pvalue"], st["lrt_pvalue"])
    else:
        engine.glm_setup(st["y"], st["W"], st["continuous"], st["llf"], st["firth_null"], st["filter_pvalue"], st["lrt_pvalue"])
    engine.set_dedup(not st["no_dedup"])
    if st["lin"] is not None:
        engine.lineage_setup(st["lin"], st["lin_cov"])
    if st["af_filter"] is not None:
        # blocks of the native reader / the packed cache hand every parsed row to the engine (input.py _block_from_raw): the AF window is applied
        # on the device as well, so filtered rows are neither copied out on the host nor contracted on the GPU
        engine.set_af_filter(*st["af_filter"])


# ---- the plan ----------------------------------------------------------------------------------------------------------------------------------
# The decisions of a run: devices (of --gpus; None without it: the single --gpu), proc_mode (one process per device), the readers, the route of the blocks
RunPlan = collections.namedtuple("RunPlan", "devices proc_mode var_type native native_vcf native_rtab dev_inflate dev_reader "
                                 "job_path lmm_block_lineage job_block job_ahead want_pat cache_selected packed_c_loop calls_job")


def make_plan(options, route, stdout_fd, patterns_fd=True, cache_selected=False, lanes=None, proc_mode=None):
    """The plan from the options, the route reader (_route.route) and the facts that need the outside world: whether stdout and the pattern file, if
    any, have a descriptor; whether --load-packed names a cache over other samples (validate_loaded); the lanes of the first context, None where
    this process has no context.  main() plans before a context exists -- for the devices, proc_mode and the readers -- and again behind the
    header line, once --packed-cache has named its file, with proc_mode as it was decided."""
    devices = _route.device_list(options.gpus)
    # One PROCESS per device for a `--gpus` job over a packed cache (round 6; pyseer_amd/_packed_child.py): this process does the host set-up
    # and joins the parts, every device's process runs the library's own block loop over its range of the cache.  SEERHIP_ROUTE procs=0: the
    # devices' streams as threads of this process (round 5).
    if proc_mode is None:
        proc_mode = bool(devices and len(devices) > 1 and options.load_packed and not options.save_packed and not options.python_sink and not options.serial_sink
                         and not options.packed_part and route("job", "1") not in ("0", "py") and route("procs", "1") != "0" and stdout_fd)
    var_type = "kmers" if options.kmers else ("vcf" if options.vcf else ("calls" if options.load_calls else "Rtab"))
    reader = not options.python_reader
    # --device-reader (SEERHIP_ROUTE kmer_dev=1): the sample tokens are read on the first context's device, on a stream of the reader's own
    # --device-inflate (SEERHIP_ROUTE kmer_inflate=1): that reader's BGZF members are decoded there too, on another stream of its own
    dev_inflate = bool(options.device_inflate or route("kmer_inflate", "0") == "1")
    dev_reader = bool((options.device_reader or dev_inflate or route("kmer_dev", "0") == "1") and options.gpus is None)
    # (the Rtab reader is bound to one context: --gpus keeps the line-by-line reader, and so does a run that names a packed cache)
    native_rtab = bool(var_type == "Rtab" and reader and options.gpus is None and not (options.load_packed or options.save_packed or options.packed_cache or options.packed_part))
    native = var_type == "kmers" and reader
    # ---- the job stream (round 5; include/seerhip.h sh_job_*): unless a cross-check sink is asked for (round 6: --lineage, --output-patterns and --print-samples
    # run inside the stream too: sh_job_set_lineage / _patterns / _samples) a block goes to the library as parsed and comes back as the text of its printed rows: the AF
    # window, the NaN masks, the counters and the choice of rows run on the device, the host formats printed rows only.  Output without
    # --print-filtered does not depend on where blocks end, so short blocks are coalesced (a 3000-row block is 90 us of GPU time).
    # --device-calls (SEERHIP_ROUTE calls_job=1; round 20): the native VCF reader's blocks (text, BCF, burden regions) and the native Rtab reader's go to the
    # job stream as parsed -- planes with missing calls, counts, skip reasons (sh_job_submit_calls) -- instead of through _vcf_packed_block and the
    # sinks of the Python block loop.  An option: the default route of these inputs is what it was.
    native_vcf = bool(var_type == "vcf" and reader)
    # --load-calls (round 21): the stored CallBlocks of a call cache take that route by default -- as stored (a cache over the run's own samples), or
    # with their planes restricted to the run's samples on the device on the way in (sh_job_submit_calls_select; cache_selected)
    calls_job = bool(((native_vcf or native_rtab) and (options.device_calls or route("calls_job", "0") == "1") and options.gpus is None) or options.load_calls)
    job_path = bool((native or options.load_packed or calls_job) and not options.python_sink and not options.serial_sink and route("job", "1") != "0")
    calls_job = calls_job and job_path
    # (--lineage, round 6: fit_lineage_effect runs inside the stream, for printed rows -- sh_job_set_lineage.  The LMM's lineage is that of each
    # block's LAST variant (pyseer/lmm.py:209-213, the stale `k`), so its blocks must end where the reference's do: no coalescing)
    lmm_block_lineage = bool(options.lineage and options.lmm and not options.lmm_lineage_per_variant)
    # (2^18 rows: a call of 2^16 runs the LMM 7 % slower, the logistic path 27 %, Firth 15 % -- profiles/r06/rows_per_call.txt; round 5 had 2^16)
    # (call blocks are read whole before they are submitted, two planes each, and several are in flight: 2^14 rows -- 21 MB at N = 5000)
    job_block = options.block_size if (options.print_filtered or lmm_block_lineage or not job_path) else max(options.block_size, 1 << (14 if calls_job else 18))
    # the reader runs as far ahead as the job stream holds blocks in flight (fixed effects: 2 + lanes, include/seerhip.h sh_job_depth)
    job_ahead = (2 + lanes) if (job_path and not options.lmm and lanes is not None) else 2
    # --count-patterns: the set of distinct patterns on the first (the only) device.  The job stream inserts every tested row there itself
    # (sh_job_set_pattern_count: no md5); the other routes make hash_pattern on the host, and the 16 digest bytes are the keys -- so are those
    # of rows with missing calls, which never reach the device (a row with a NaN never equals one without: the count stays exact)
    want_pat = bool(options.output_patterns) or bool(options.count_patterns and not job_path)
    # a packed cache through the job stream: the block loop runs inside the library, one call per device (SEERHIP_ROUTE job=py: the loop in
    # Python, as round 5 had it and as text input still has it)
    # (the library's loop takes a cache of the run's own samples only: a selected cache goes through the Python loop)
    packed_c_loop = bool(job_path and options.load_packed and not cache_selected and route("job", "1") != "py" and stdout_fd and patterns_fd)
    return RunPlan(devices, proc_mode, var_type, native, native_vcf, native_rtab, dev_inflate, dev_reader,
                   job_path, lmm_block_lineage, job_block, job_ahead, want_pat, bool(cache_selected), packed_c_loop, calls_job)


# ---- the run's context and its input -----------------------------------------------------------------------------------------------------------
class RunContext(object):
    """What the runners of one run share.  state: model_state (the engines' and the Jobs' set-up, the names list of --print-samples) -- a device's
    process fills in that alone; p: the phenotypes, cut down to the run's samples, pv: their values; lineage_dict: None without --lineage;
    count_set: the PatternSet of --count-patterns; patterns: the --output-patterns file.  For report_cli the runners leave here: tms, one timing
    dict per stream (new_tm); thread_cpu, the CPU seconds of the block loop's Python threads by role (time.thread_time); child_budget; marks."""
    def __init__(self, state, options=None, p=None, pv=None, model=None, lineage_dict=None, plan=None, engs=(), count_set=None, patterns=None):
        self.state, self.options, self.p, self.pv, self.model, self.lineage_dict = state, options, p, pv, model, lineage_dict
        self.plan, self.engs, self.count_set, self.patterns = plan, engs, count_set, patterns
        self.tms, self.thread_cpu, self.child_budget, self.marks = None, {}, None, None


def make_job(ctx, engine, patterns):
    st = ctx.state
    return Job(engine, st["lmm"], st["print_filtered"], lineage_labels=st["lineage_labels"], lineage_per_variant=st["lineage_per_variant"],
               patterns=patterns, sample_names=st["sample_names"], pattern_count=ctx.count_set is not None)


def prepare_input(options, plan, p):
    """What is opened and checked before the header line: the burden regions, the gzip check, the Python readers' file."""
    from .input import check_kmers_gzipped, load_burden, open_variant_file
    kmer_files = list(options.kmers) if options.kmers else []
    src = SimpleNamespace(kmer_files=kmer_files, var_file=(kmer_files[0] if kmer_files else (options.vcf or options.pres or options.load_calls)), infile=None,
                          sample_order=None, burden_regions=(collections.deque([]) if options.burden else None), cache_out=None, calls_out=None, selector=None, call_cache=None)
    if options.load_calls:
        src.call_cache = open_run_call_cache(options.load_calls, p)
    if plan.native and not options.uncompressed and not options.load_packed:
        check_kmers_gzipped(kmer_files or [src.var_file])
    if options.save_calls and plan.native_rtab:
        # (a header that names a phenotype sample twice is read line by line, the last call that is not `0` winning: no planes to store.  The native
        # reader's own refusal, asked for here, before the header line, by opening it without a device)
        from .input import NativeRtabReader, RtabDuplicateSample
        try:
            NativeRtabReader(src.var_file, [str(x) for x in p.index], None, 1).close()
        except RtabDuplicateSample as ex:
            die("--save-calls needs the native Rtab reader, which does not read %s (%s)\n" % (src.var_file, ex))
    if plan.native_vcf:
        if options.burden:
            load_burden(options.burden, src.burden_regions)
    elif not plan.native and not plan.native_rtab and not options.load_calls:
        src.infile, src.sample_order = open_variant_file(plan.var_type, src.var_file, options.burden, src.burden_regions, options.uncompressed)
    return src


def print_header(options, cov):
    header = ['variant', 'af', 'filter-pvalue', 'lrt-pvalue', 'beta', 'beta-std-err']
    if options.lmm:
        header.append('variant_h2')
    else:
        header += ['intercept'] + ([] if options.no_distances else ['PC%d' % i for i in range(1, options.max_dimensions + 1)])
        header += [x for x in cov.columns] if options.covariates is not None else []
    header += (['lineage'] if options.lineage else []) + (['k-samples', 'nk-samples'] if options.print_samples else []) + ['notes']
    print('\t'.join(header))


def open_blocks(ctx, src, cache_stamp=None, part=None, eng=None):
    """The run's block iterator (input.py); --save-packed's writer is left in src.cache_out.  part, eng: range i of n of a packed cache, for that context."""
    from . import input as I
    options, plan, p, engs = ctx.options, ctx.plan, ctx.p, ctx.engs
    af = (options.min_af, options.max_af)
    if options.load_packed:
        eng = eng if eng is not None else (engs[0] if engs else None)
        return I.iter_packed_blocks_cached(p, options.load_packed, *af, plan.job_block, want_patterns=plan.want_pat, want_samples=options.print_samples, part=part,
                                           raw=plan.job_path, device=(eng.device if (plan.job_path and eng is not None) else None), ahead=plan.job_ahead,
                                           select=(eng if plan.cache_selected else None))
    if plan.native and len(src.kmer_files) > 1:
        return I.iter_packed_blocks_native_multi(p, src.kmer_files, *af, plan.job_block, want_patterns=plan.want_pat, want_samples=options.print_samples, raw=plan.job_path)
    if plan.native:
        if options.save_packed:
            src.cache_out = I.PackedCacheWriter(options.save_packed, [str(x) for x in p.index], stamp=cache_stamp)
        return I.iter_packed_blocks_native(p, src.var_file, *af, plan.job_block, want_patterns=plan.want_pat, want_samples=options.print_samples, save_to=src.cache_out,
                                           raw=plan.job_path, engine=(engs[0] if (plan.dev_reader and engs) else None), inflate=(True if options.device_inflate else None))
    if options.load_calls:
        # a call cache: as stored for the run's own sample list; else restricted to the run's samples -- inside the job stream (fused: the blocks go up
        # over the stored samples, behind the selector kept in src until the run ends), or block by block before they are handed on
        found, stored_blocks, sample_map = src.call_cache
        mode, how = ("job" if plan.job_path else "packed"), call_cache_select_mode()
        if sample_map is not None and how != "host":
            from .engine import RowSelector
            src.selector = RowSelector(engs[0], len(found), sample_map)
            if plan.job_path and how == "fused":
                mode = "fused"
        return I.iter_call_cache_blocks(p, stored_blocks, plan.job_block, mode, src.selector, len(found), sample_map, options.max_missing, *af,
                                        want_patterns=plan.want_pat)
    if options.save_calls and (plan.native_vcf or plan.native_rtab):
        src.calls_out = I.CallCacheWriter(options.save_calls, [str(x) for x in p.index], options.block_size)
    if plan.calls_job and plan.native_vcf:
        # (the reader and the job stream share the first context: the blocks are read on the thread that submits them, between its calls)
        return I.iter_job_call_blocks_vcf(p, src.var_file, engs[0], plan.job_block, burden_regions=(list(src.burden_regions) if options.burden else None),
                                          save_to=src.calls_out)
    if plan.calls_job:
        try:
            return I.iter_job_call_blocks_rtab(I.NativeRtabReader(src.var_file, [str(x) for x in p.index], engs[0], plan.job_block), save_to=src.calls_out)
        except I.RtabDuplicateSample:
            # a header that names a sample twice is read line by line (iter_packed_blocks_rtab_native), through the Python block loop
            ctx.plan = plan = plan._replace(calls_job=False, job_path=False, job_block=options.block_size, want_pat=bool(options.output_patterns or options.count_patterns))
    if plan.native_vcf:
        # the reader uses the first context's device and stream between that context's own calls (one stream: the order is the stream's)
        return I.iter_packed_blocks_vcf_native(p, src.var_file, engs[0], *af, options.max_missing, options.block_size,
                                               burden_regions=(list(src.burden_regions) if options.burden else None), save_to=src.calls_out)
    if plan.native_rtab:
        # (as above: the calls are tokenised on the first context's device; a header that names a sample twice takes the line reader by itself)
        return I.iter_packed_blocks_rtab_native(p, src.var_file, engs[0], *af, options.max_missing, options.block_size, save_to=src.calls_out)
    return I.iter_packed_blocks(p, plan.var_type, src.infile, set(p.index), src.sample_order, *af, options.max_missing, options.uncompressed,
                                options.block_size, burden=bool(options.burden), burden_regions=src.burden_regions)


# ---- the runners -------------------------------------------------------------------------------------------------------------------------------
class Counts(object):
    """(pre-filtered, tested, printed) of one stream"""
    prefilter = tested = printed = 0

    def done(self, tm, **more):
        tm.update(rows=self.prefilter + self.tested, loop=time.perf_counter() - tm["t0"], **more)
        return self.prefilter, self.tested, self.printed


def new_tm():
    return {"engine": 0.0, "sink": 0.0, "write": 0.0, "blocks": 0, "t0": time.perf_counter(), "reader": 0.0, "queue": 0.0, "format": 0.0, "t0w": time.time(), "rows": 0}


def run_stream_job(ctx, engs, blocks, write_text, tm, stop=None, write_patterns=None):
    """One stream of RawBlocks (or, --device-calls, CallBlocks) through the library's job stream, block k on context k % len(engs) (each context pipelined Job.depth deep: the rows of its next block cross
    PCIe while the block before runs its kernels and the one before that is written out here). Returns (pre-filtered, tested, printed)."""
    jobs = [make_job(ctx, e_, write_patterns is not None) for e_ in engs]
    n = Counts()
    order = collections.deque()                           # the job each block in flight went to, in input order

    def take():
        jb = order.popleft()
        t_c = time.perf_counter()
        text, cnt, release = jb.collect()
        tm["engine"] += time.perf_counter() - t_c
        if getattr(release, "selector", None) is not None:
            # a block of a call cache selected inside the stream: its counts over the run's samples exist now, and with them what say_call_block says
            from .input import say_call_block
            release.n_present, release.n_missing = jb.calls_counts()
            say_call_block(release)
            release = None
        n.prefilter += cnt[0]; n.tested += cnt[1]; n.printed += cnt[2]
        if write_patterns is not None and cnt[1]:
            write_patterns(jb.patterns())                 # (hash_pattern of the block's tested variants, made on the device)
        if len(text):
            t_w = time.perf_counter()
            write_text(text)
            tm["write"] += time.perf_counter() - t_w
        if release is not None:
            release()
    try:
        blocks = iter(blocks)
        k = 0
        while True:
            t_r = time.perf_counter()
            rb = next(blocks, None)                       # (waiting here = the reader is the slowest stage)
            tm["reader"] += time.perf_counter() - t_r
            if rb is None or (stop is not None and stop.is_set()):
                break
            jb = jobs[k % len(jobs)]
            while jb.pending() >= jb.depth:
                take()
            t_e = time.perf_counter()
            if getattr(rb, "selector", None) is not None:  # a stored block of a call cache over other samples (input.iter_call_cache_blocks, "fused")
                jb.submit_calls_select(rb.selector, rb.present, rb.missing, rb.skip, rb.blob, rb.off, ctx.options.max_missing, keep=rb)
            elif getattr(rb, "missing", None) is not None:  # a CallBlock of the native VCF / Rtab reader (input.iter_job_call_blocks_*)
                jb.submit_calls(rb.present, rb.missing, rb.n_present, rb.n_missing, rb.skip, rb.blob, rb.off, ctx.options.max_missing)
            else:
                jb.submit(rb.bits, rb.counts, rb.blob, rb.off, rows_are_dma=rb.dma, keep=rb.release)
            tm["engine"] += time.perf_counter() - t_e; tm["blocks"] += 1
            order.append(jb)
            # depth - 1 blocks stay in flight per context (one uploading, one computing per lane); the next is collected, formatted and written
            while len(order) > (jobs[0].depth - 1) * len(jobs):
                take()
            k += 1
        while order:
            take()
    finally:
        for jb in jobs:
            jb.close()
    return n.done(tm, overlap=True, job=True)


def run_stream_packed(ctx, eng, part, out_file, pat_file, tm, stop_c=None):
    """One stream of a packed cache entirely inside the library (round 6: sh_job_run_packed -- csrc/job_run.inc): the block loop, the DMA
    windows, the writes to the two descriptors; this thread holds no interpreter lock while it runs."""
    for f in (sys.stdout, out_file, pat_file):             # (the header line sits in the text layer's buffer)
        if f is not None:
            f.flush()
    job = make_job(ctx, eng, pat_file is not None)
    try:
        pf_, te_, pr_, nb_ = job.run_packed(ctx.options.load_packed, part, ctx.plan.job_block, use_dma=_route.route("dma", "1") != "0", out_fd=out_file.fileno(),
                                            pat_fd=(pat_file.fileno() if pat_file is not None else -1), stop=stop_c)
    finally:
        job.close()
    tm.update(blocks=nb_, rows=pf_ + te_, loop=time.perf_counter() - tm["t0"], overlap=True, job=True)
    tm["engine"] = tm["loop"]
    return pf_, te_, pr_


def last_variant_lineage(blk, eng):
    """--lmm --lineage as the reference has it (pyseer/lmm.py:209-213): inside fit_lmm's second loop `k` still holds the LAST variant unpacked
    by the first loop, so every passing variant of a block reports the lineage of that last variant.  -> its index, -1 for none."""
    kl = blk.last_k
    if kl is None or np.isnan(np.asarray(kl, dtype=float)).any():
        return -1
    return int(eng.lineage_batch(pack_variants(np.asarray(kl).reshape(1, -1)))[0])


def _unfitted(lmm, name, pattern, af, prep, ks, nks, notes, prefilter, filter_, nan=np.nan):
    if lmm:
        return LMM(name, pattern, af, prep, nan, nan, nan, nan, None, ks, nks, notes, prefilter, filter_)
    return Seer(name, pattern, af, prep, nan, nan, nan, nan, np.array([]), None, ks, nks, notes, prefilter, filter_)


def _fitted(lmm, name, pattern, af, r, j, ks, nks):
    fl = int(r["flags"][j])
    notes, pf, ft = notes_from_flags(fl), bool(fl & FLAG_PREFILTER), bool(fl & FLAG_FILTER)
    if lmm:
        return LMM(name, pattern, af, r["prep"][j], r["pvalue"][j], r["beta"][j], r["bse"][j], r["frac_h2"][j], None, ks, nks, notes, pf, ft)
    tested_ok = np.isfinite(r["kbeta"][j]) or np.isfinite(r["pvalue"][j])
    betas = r["betas"][j] if (tested_ok and r["betas"].shape[1]) else np.array([])
    return Seer(name, pattern, af, r["prep"][j], r["pvalue"][j], r["kbeta"][j], r["bse"][j], r["intercept"][j], betas, None, ks, nks, notes, pf, ft)


def rows_of_block(ctx, blk, r):
    """The reference's row objects of one block, in input order (None: a skipped VCF record); r: the engine's results, masked for the LMM."""
    options = ctx.options
    rows = []
    for i, name in enumerate(blk.names):
        st, af, ks, nks = blk.status[i], blk.afs[i], blk.kstrains[i], blk.nkstrains[i]
        if st == 3:                                   # a skipped VCF record: loaded and pre-filtered (input.py:608, :693), never a row
            rows.append(None)
        elif st == 1:                                   # AF / missing filtered (model.py:255-260, lmm.py:160-167)
            rows.append(_unfitted(options.lmm, name, None if options.lmm else blk.patterns[i], af, np.nan, ks, nks, {'af-filter'}, True, False))
        elif st == 2:                                   # missing calls inside k: the reference's error path
            prep, bad = host_pre_filtering(ctx.pv, blk.ks[i], options.continuous)
            notes = {'bad-chisq'} if bad else set()
            thr = options.filter_pvalue
            failed = (prep >= thr) if options.lmm else (prep > thr)
            prefiltered = bool(failed or not np.isfinite(prep))
            if prefiltered:
                notes.add('pre-filtering-failed')
            else:                                     # NaN propagates through fit_lmm_block; statsmodels MissingDataError, model.py:371-377
                notes.add('lrt-filtering-failed' if options.lmm else 'missing-data-error')
            rows.append(_unfitted(options.lmm, name, blk.patterns[i], af, prep, ks, nks, notes, prefiltered, not prefiltered))
        else:
            rows.append(_fitted(options.lmm, name, blk.patterns[i], af, r, blk.row_of[i], ks, nks))
    return rows


class BlockSink(object):
    """The ordered sink of one stream: block sink (csrc/writer.cpp) -- results stay arrays from the engine to the TSV text; the per-variant
    tuple path is kept for --print-samples, for variants carrying missing calls, and as the cross-check (--python-sink).
    The array sink runs on a worker thread (NaN masking, counters, native formatter, the write to stdout -- the reference does all of this per
    variant between two fits, pyseer/__main__.py:805-827).  One worker and a FIFO of depth 2: the output order is the input order.  The tuple
    path and the lineage fits (a second engine call on the same context) stay on the caller's thread, after the worker has drained."""
    def __init__(self, ctx, write_text, write_patterns, tm):
        options = ctx.options
        self.ctx, self.options, self.tm, self.n = ctx, options, tm, Counts()
        self.write_text, self.write_patterns = write_text, write_patterns
        self.formatter = RowFormatter(ctx.lineage_dict if options.lineage else None)     # (its text buffer is valid until its next call: one per stream)
        self.q, self.err = queue.Queue(maxsize=2), []
        self.overlap = not options.lineage and not options.python_sink and not options.print_samples and not options.serial_sink
        self.thread = threading.Thread(target=self._worker, daemon=True) if self.overlap else None
        if self.overlap:
            self.thread.start()

    def _worker(self):
        while True:
            item = self.q.get()
            try:
                if item is None:
                    return
                if not self.err:
                    self.sink_block(*item)
            except BaseException as ex:          # re-raised on the main thread
                self.err.append(ex)
            finally:
                self.q.task_done()

    def drain(self):
        if self.thread is not None:
            self.q.join()
        if self.err:
            raise self.err[0]

    def close(self):
        self.drain()
        if self.thread is not None:
            self.q.put(None)
            self.thread.join()

    def put(self, blk, r, eng):
        """Everything that follows a block's engine call: the array sink, or the reference's row objects.  eng: the context that holds the block's rows (the lineage fits go there)."""
        options = self.options
        if options.python_sink or options.print_samples or 2 in blk.status:
            self.drain()
            self.sink_rows(blk, r, eng)
        elif self.overlap:
            if self.err:
                raise self.err[0]
            t_q = time.perf_counter()
            self.q.put((blk, r, eng))                 # (waiting here = the sink is the slowest stage)
            self.tm["queue"] += time.perf_counter() - t_q
        else:
            self.sink_block(blk, r, eng)

    def sink_block(self, blk, r, eng):
        options, n, tm = self.options, self.n, self.tm
        if options.lmm and r is not None:
            r = mask_like_fit_lmm(r)
        t_in = time.perf_counter()
        nb = len(blk)
        status = np.asarray(blk.status)
        on = status == 0
        row_of = np.asarray(blk.row_of, dtype=np.int64)
        # blocks of the native reader / the packed cache: one engine row per variant, in place (row_of = 0, 1, 2, ...): whole-array selects
        # instead of gathers through an index
        ident = r is not None and isinstance(blk.row_of, np.ndarray) and nb == r["flags"].shape[0]
        j = None if ident else row_of[on]
        flags = np.zeros(nb, dtype=np.uint32)
        flags[(status == 1) | (status == 3)] = NOTE_AF | FLAG_PREFILTER
        keys = ("prep", "pvalue", "beta", "bse", "frac_h2") if options.lmm else ("prep", "pvalue", "kbeta", "bse", "intercept")
        cols = [np.asarray(blk.afs, dtype=np.float64)]
        for kname in keys:
            if ident:
                c = np.where(on, r[kname], np.nan)
            else:
                c = np.full(nb, np.nan)
                if r is not None:
                    c[on] = r[kname][j]
            cols.append(c)
        betas = valid = None
        if r is not None:
            if ident:
                flags = np.where(on, r["flags"], flags)
            else:
                flags[on] = r["flags"][j]
            if not options.lmm and r["betas"].shape[1]:
                if ident:
                    betas = r["betas"]                    # (rows that are not `on` have valid = 0: the formatter never reads their slopes)
                    valid = (on & (np.isfinite(r["kbeta"]) | np.isfinite(r["pvalue"]))).astype(np.uint8)
                else:
                    betas = np.full((nb, r["betas"].shape[1]), np.nan)
                    betas[on] = r["betas"][j]
                    valid = np.zeros(nb, dtype=np.uint8)
                    valid[on] = np.isfinite(r["kbeta"][j]) | np.isfinite(r["pvalue"][j])
        pf = (flags & FLAG_PREFILTER) != 0
        ft = (flags & FLAG_FILTER) != 0
        lineage = None
        if options.lineage:
            lineage = np.full(nb, -1, dtype=np.int32)
            if options.lmm and not options.lmm_lineage_per_variant:
                lineage[~pf & ~ft] = last_variant_lineage(blk, eng)
            else:
                need = on & ~pf & (~ft if options.lmm else ((flags & NOTE_FIRTH_FAIL) == 0))
                if need.any():
                    lineage[need] = eng.lineage_batch(blk.bits[row_of[need]])
        order = np.arange(nb)
        if options.lmm:                                   # fit_lmm's return order: filtered first, then tested
            order = np.concatenate([order[pf], order[~pf]])
        npf = int(pf.sum())
        n.prefilter += npf
        n.tested += nb - npf
        if self.write_patterns is not None:
            self.write_patterns(b''.join(blk.patterns[i] for i in order if not pf[i]))
        show = (status != 3) if options.print_filtered else (~pf & ~ft)      # (a skipped VCF record has no name: counted, never a row)
        sel = order[show[order]]
        n.printed += int(sel.shape[0])
        if sel.shape[0]:
            blob, off = (blk.names_blob, blk.name_off) if getattr(blk, "names_blob", None) is not None else names_blob(blk.names)
            t_f = time.perf_counter()
            text = self.formatter.format_view(blob, off, sel, cols, flags, betas, valid, lineage)
            t_w = time.perf_counter()
            tm["format"] += t_w - t_f
            self.write_text(text)
            tm["write"] += time.perf_counter() - t_w
        tm["sink"] += time.perf_counter() - t_in

    def sink_rows(self, blk, r, eng):
        """The tuple path: one row object per variant, formatted in Python."""
        options = self.options
        if options.lmm and r is not None:
            r = mask_like_fit_lmm(r)
        rows = rows_of_block(self.ctx, blk, r)
        if options.lineage:
            # fit_lineage_effect: fixed effects -> every variant that reached the fit (model.py:379-382; firth-fail and
            # missing-data return earlier); LMM -> only variants that pass the LRT filter (lmm.py:209-213)
            need = [i for i, x in enumerate(rows) if x is not None and blk.status[i] == 0 and not x.prefilter and
                    ((not x.filter) if options.lmm else ('firth-fail' not in x.notes))]
            if options.lmm and not options.lmm_lineage_per_variant:
                ml = last_variant_lineage(blk, eng)
                for i, x in enumerate(rows):
                    if x is not None and not x.prefilter and not x.filter:
                        rows[i] = x._replace(max_lineage=(None if ml < 0 else ml))
            elif need:
                ml = eng.lineage_batch(blk.bits[[blk.row_of[i] for i in need]])
                for i, v in zip(need, ml):
                    rows[i] = rows[i]._replace(max_lineage=(None if v < 0 else int(v)))
        self.n.prefilter += sum(1 for x in rows if x is None)
        rows = [x for x in rows if x is not None]
        if options.lmm:                                   # fit_lmm's return order: filtered first, then tested
            rows = [x for x in rows if x.prefilter] + [x for x in rows if not x.prefilter]
        n = self.n
        for x in rows:
            if x.prefilter:
                n.prefilter += 1
            else:
                n.tested += 1
                if self.write_patterns is not None:
                    self.write_patterns(x.pattern)
            if options.print_filtered or not (x.prefilter or x.filter):
                n.printed += 1
                self.write_text((format_output(x, self.ctx.lineage_dict, self.ctx.model, options.print_samples) + "\n").encode())


def run_stream(ctx, engs, blocks, write_text, write_patterns, tm):
    """One stream of blocks, in order: reader (its own thread inside `blocks`) -> engine calls, block k on engs[k % len(engs)], each engine pipelined -> one ordered sink
    writing through write_text / write_patterns.  Returns (pre-filtered, tested, printed).  The job runs one such stream per device when the input can be cut into ranges (a
    packed cache), else one stream over all devices. Three stages run at once (round 3): the block reader (its own thread, `prefetched`), the engine call of block k on this
    thread (a ctypes call: the GIL is released while the rows go to the GPU and the statistics come back), and the sink of block k-1 (BlockSink). The engine calls
    themselves are pipelined (sh_*_batch_async, include/seerhip.h): a call returns while its last chunk is still on the device, and that chunk's results arrive while the
    NEXT call on the same context stages and queues its first chunk -- a block is therefore handed on len(engs) iterations late.  Synchronous calls left the device idle for
    a third of every call (first chunk's staging + upload at the head, the last chunk's kernels + download at the tail: 12.6 ms per 262 144-row block of which 8 ms were
    kernels).  With one context the loop also announces the rows of the block it has read ahead (sh_prefetch_rows)."""
    sink = BlockSink(ctx, write_text, write_patterns, tm)
    lmm = ctx.options.lmm
    G = len(engs)
    pend = collections.deque()                        # (block, results, engine) handed to the engine, not yet to the sink
    blocks = iter(blocks)
    t_r = time.perf_counter()
    ahead = next(blocks, None)
    tm["reader"] += time.perf_counter() - t_r
    k = 0
    while ahead is not None:
        blk = ahead
        t_r = time.perf_counter()
        ahead = next(blocks, None)                    # (waiting here = the reader is the slowest stage)
        tm["reader"] += time.perf_counter() - t_r
        t_e = time.perf_counter()
        e = engs[k % G]
        r = None
        if G == 1 and ahead is not None and ahead.bits.shape[0] and ahead.bits.dtype == np.uint8 and ahead.bits.flags.c_contiguous:
            e.prefetch(ahead.bits)                    # block k+1's first chunk goes up while block k is on the device (sh_prefetch_rows)
        if blk.bits.shape[0]:
            r = e.lmm_batch(blk.bits, pipelined=True) if lmm else e.glm_batch(blk.bits, pipelined=True)
        else:
            e.wait()                                  # no call for an empty block: complete this context's previous one here
        tm["engine"] += time.perf_counter() - t_e; tm["blocks"] += 1
        pend.append((blk, r, e))
        # block j is complete once its context has returned from its next call (or wait): the oldest of more than G pending ones is
        while len(pend) > G:
            sink.put(*pend.popleft())
        k += 1
    while pend:
        b_, r_, e_ = pend.popleft()
        t_e = time.perf_counter()
        e_.wait()
        tm["engine"] += time.perf_counter() - t_e
        sink.put(b_, r_, e_)
    sink.close()
    return sink.n.done(tm, overlap=sink.overlap)


class _CountKeys(object):
    """--count-patterns outside the job stream: the pattern lines on their way to the --output-patterns file, if any, are the keys of the set
    (the tuple path writes one line per variant: the keys go to the device in batches)."""
    def __init__(self, count_set, to_file):
        self.count_set, self.to_file, self.held = count_set, to_file, []

    def write(self, b):
        if self.to_file is not None:
            self.to_file(b)
        if len(b):
            self.held.append(bytes(b))
            if len(self.held) >= 4096 or len(b) >= 25 * 4096:
                self.flush()

    def flush(self):
        from .count_patterns import digests_of_lines
        if self.held:
            self.count_set.add_keys(digests_of_lines(b''.join(self.held)))
            del self.held[:]


def run_processes(ctx):
    """One process per device (pyseer_amd/_packed_child.py) over its range of the cache; this one joins their parts and sums their counters."""
    from .input import check_packed_cache
    options, plan, patterns = ctx.options, ctx.plan, ctx.patterns
    check_packed_cache(ctx.p, options.load_packed)
    devs, G = plan.devices, len(plan.devices)
    state_dir = tempfile.mkdtemp(prefix="pyseer_amd_job_")
    try:
        write_state(state_dir, dict(ctx.state, devices=devs, patterns=patterns is not None, job_block=int(plan.job_block),
                                    dma=_route.route("dma", "1") != "0", path=os.path.abspath(options.load_packed)))
        sys.stdout.flush()
        env_c = dict(os.environ)
        env_c["PYTHONPATH"] = os.path.dirname(os.path.dirname(os.path.abspath(__file__))) + os.pathsep + env_c.get("PYTHONPATH", "")
        t_children0 = time.perf_counter()
        kids = [subprocess.Popen([sys.executable, "-m", "pyseer_amd._packed_child", state_dir, str(i)], env=env_c,
                                 stdout=(None if i == 0 else subprocess.DEVNULL), stderr=subprocess.PIPE) for i in range(G)]
        # (like the reference's and the single-device run's, the output of a run that fails is partial: what part 0 had printed)
        errs_c = [k_.communicate()[1].decode() for k_ in kids]
        for err_ in errs_c:
            for line in err_.splitlines():
                if line.startswith("No observations of ") or line.startswith("pyseer_amd:"):
                    sys.stderr.write(line + "\n")
        bad = [i for i, k_ in enumerate(kids) if k_.returncode != 0]
        if bad:
            sys.stderr.write(errs_c[bad[0]][-4000:])
            die("pyseer_amd: the stream of device %d failed; the output is partial\n" % devs[bad[0]])
        results = []
        for i in range(G):
            with open(os.path.join(state_dir, "result_%d.json" % i)) as fh:
                results.append(json.load(fh))
        join_parts((open(os.path.join(state_dir, "out_%d.tsv" % i), "rb") for i in range(1, G)), write_stdout)
        if patterns is not None:
            patterns.flush()
            join_parts((open(os.path.join(state_dir, "pat_%d.txt" % i), "rb") for i in range(G)), patterns.write)
        ctx.tms = []
        for i, r_ in enumerate(results):
            tm_ = new_tm(); tm_.update(blocks=r_["blocks"], rows=r_["prefilter"] + r_["tested"], loop=r_["wall_s"], engine=r_["wall_s"], overlap=True, job=True)
            ctx.tms.append(tm_)
            ctx.thread_cpu["device %d process (block loop, user + sys)" % devs[i]] = r_["user_s"] + r_["sys_s"]
        ctx.child_budget = {"user_s": sum(r_["user_s"] for r_ in results), "sys_s": sum(r_["sys_s"] for r_ in results),
                            "stages": {k_: sum(r_["library_stage_cpu_s"].get(k_, 0.0) for r_ in results) for k_ in results[0]["library_stage_cpu_s"]},
                            "wall_s": max(r_["wall_s"] for r_ in results), "launch_to_join_s": time.perf_counter() - t_children0}
        return tuple(sum(r_[k_] for r_ in results) for k_ in ("prefilter", "tested", "printed"))
    finally:
        shutil.rmtree(state_dir, ignore_errors=True)


def run_threads(ctx):
    """One stream per context of this process, each over its range of the cache on a thread of its own (procs=0, and every --gpus run over a cache but run_processes')."""
    plan, engs, patterns, G = ctx.plan, ctx.engs, ctx.patterns, len(ctx.engs)
    _abi.load().sh_set_host_streams(G)                     # per-stream helpers (stager, readers) take 1/G of the host CPU budget each
    ctx.tms = tms = [new_tm() for _ in range(G)]
    # part 0 goes straight to stdout, the others to temporary files ($TMPDIR) joined in order at the end: like the reference's and the
    # single-device run's, the output of a run that fails is partial (what part 0 had printed); the first error stops the other streams
    outs = [binary_stdout()] + [tempfile.TemporaryFile() for _ in range(1, G)]
    pouts = [patterns] + [tempfile.TemporaryFile() if patterns is not None else None for _ in range(1, G)]
    counts, errs = [None] * G, [None] * G
    stop = threading.Event()
    stop_c = ctypes.c_int(0)

    def stream_worker(i):
        try:
            t_th = time.thread_time()
            if plan.packed_c_loop:
                counts[i] = run_stream_packed(ctx, engs[i], (i, G), outs[i], pouts[i], tms[i], stop_c)
            else:
                blocks_i = open_blocks(ctx, None, part=(i, G), eng=engs[i])
                wt = write_stdout if i == 0 else outs[i].write
                wp = None if patterns is None else pouts[i].write
                if plan.job_path:
                    counts[i] = run_stream_job(ctx, [engs[i]], blocks_i, wt, tms[i], stop, wp)
                else:
                    counts[i] = run_stream(ctx, [engs[i]], blocks_i, wt, wp, tms[i])
            ctx.thread_cpu["stream %d loop thread" % i] = time.thread_time() - t_th
        except BaseException as ex:                    # re-raised below, on the main thread
            errs[i] = ex
            stop.set()
            stop_c.value = 1
    workers = [threading.Thread(target=stream_worker, args=(i,)) for i in range(G)]
    for w_ in workers:
        w_.start()
    for w_ in workers:
        w_.join()
    for ex in errs:
        if ex is not None:
            raise ex
    join_parts(outs[1:], write_stdout)
    if patterns is not None:
        join_parts(pouts[1:], patterns.write)
    return tuple(sum(c[j] for c in counts) for j in range(3))


def run(ctx, blocks):
    """The block loop, the way the plan says.  Returns (pre-filtered, tested, printed); the timings are left in ctx for report_cli. The reference's --cpu N hands blocks of
    the variant stream to N workers and takes them back in order (__main__.py:541-568, 777-780). Here every device gets its own pipelined stream when the input can be cut
    into ranges up front (the packed cache: range i of the rows to context i, each with its own reader thread, engine pipeline, sink thread and output part; the parts are
    joined in order and the four counters summed at the end -- nothing crosses between devices while the job runs).  Input that is only readable front to back (text, gzip)
    stays one stream whose blocks go to the contexts in turn."""
    options, plan, engs, patterns = ctx.options, ctx.plan, ctx.engs, ctx.patterns
    ctx.tms = [new_tm()]
    ctx.marks = {"ru": resource.getrusage(resource.RUSAGE_SELF), "stages": _abi.host_cpu_seconds(), "t": time.perf_counter(),
                 "tasks": task_cpu() if _route.debug("cli") else {}}        # where the block loop starts, for report_cli
    if plan.packed_c_loop:
        from .input import check_packed_cache
        check_packed_cache(ctx.p, options.load_packed)
    if plan.proc_mode:
        return run_processes(ctx)
    if len(engs) > 1 and options.load_packed:
        return run_threads(ctx)
    wp = None if patterns is None else patterns.write
    t_th = time.thread_time()
    if plan.packed_c_loop:
        part = tuple(int(x) for x in options.packed_part.split("/")) if options.packed_part else (0, 1)
        counts = run_stream_packed(ctx, engs[0], part, binary_stdout(), patterns, ctx.tms[0])
    elif plan.job_path:
        counts = run_stream_job(ctx, engs, blocks, write_stdout, ctx.tms[0], None, wp)
    else:
        keys = _CountKeys(ctx.count_set, wp) if ctx.count_set is not None else None
        counts = run_stream(ctx, engs, blocks, write_stdout, keys.write if keys is not None else wp, ctx.tms[0])
        if keys is not None:
            keys.flush()
        return counts                                      # (the Python block loop has never reported its thread's CPU: loop_thread_cpu_s keeps its keys)
    ctx.thread_cpu["stream 0 loop thread"] = time.thread_time() - t_th
    return counts


# ---- SEERHIP_DEBUG=cli ---------------------------------------------------------------------------------------------------------------------------
def task_cpu():
    """user / system CPU seconds of every thread of the process by name: /proc/self/task/*/stat"""
    out = {}
    try:
        tck = float(os.sysconf("SC_CLK_TCK"))
        for tid in os.listdir("/proc/self/task"):
            try:
                st = open("/proc/self/task/%s/stat" % tid).read()
            except (IOError, OSError):
                continue
            comm = st[st.index("(") + 1:st.rindex(")")]
            f = st[st.rindex(")") + 2:].split()
            out[int(tid)] = (comm, int(f[11]) / tck, int(f[12]) / tck)
    except Exception:
        pass
    return out


def report_cli(ctx, t_inputs, t_setup):
    """The `[cli budget]` and `[cli timing]` lines.  The host budget of the block loop (tools/gpu_e2e_job.py -> profiles/r05/host_budget.json): process CPU seconds
    (user + sys, every thread: getrusage) over the loop, the library's own per-stage thread CPU (csrc/host_pool.h), the loop threads' CPU (time.thread_time)."""
    tms, child, m0, lib = ctx.tms, ctx.child_budget, ctx.marks, _abi.load()
    ru1 = resource.getrusage(resource.RUSAGE_SELF); st1 = _abi.host_cpu_seconds()
    user_s, sys_s = ru1.ru_utime - m0["ru"].ru_utime, ru1.ru_stime - m0["ru"].ru_stime
    if child is not None:                                  # the block loops ran in the devices' processes: their own rusage over their loops
        user_s += child["user_s"]; sys_s += child["sys_s"]
        st1 = {k_: st1.get(k_, 0.0) + child["stages"].get(k_, 0.0) for k_ in set(st1) | set(child["stages"])}
    budget = {"rows": int(sum(tm_["rows"] for tm_ in tms)), "wall_s": (child["wall_s"] if child is not None else time.perf_counter() - m0["t"]),
              "streams": len(tms), "job_path": bool(ctx.plan.job_path), "host_cpus": int(lib.sh_host_cpus()), "pool_workers": int(lib.sh_host_pool_workers()),
              "process_cpu_s": user_s + sys_s, "process_user_s": user_s, "process_sys_s": sys_s,
              "library_stage_cpu_s": {k_: st1[k_] - m0["stages"].get(k_, 0.0) for k_ in st1}, "loop_thread_cpu_s": ctx.thread_cpu}
    by_name = {}
    for tid, (comm, ut, stt) in task_cpu().items():
        u0, s0 = m0["tasks"].get(tid, (comm, 0.0, 0.0))[1:]
        a = by_name.setdefault(comm, [0, 0.0, 0.0]); a[0] += 1; a[1] += ut - u0; a[2] += stt - s0
    budget["threads_by_name"] = {k_: {"threads": v_[0], "user_s": round(v_[1], 3), "sys_s": round(v_[2], 3)} for k_, v_ in by_name.items() if v_[1] + v_[2] >= 0.01}
    sys.stderr.write("[cli budget] " + json.dumps(budget) + "\n")
    for i, tm in enumerate(tms):
        if tm.get("job"):
            sys.stderr.write("[cli timing] stream %d of %d (job stream): %d blocks, %d rows in %.2f s of the block loop = %.3g rows/s; in library calls (submit + "
                             "collect: launches, the wait for the oldest block, formatting of printed rows) %.2f s, write %.2f s; this thread waited %.2f s for the reader\n"
                             % (i, len(tms), tm["blocks"], tm["rows"], tm["loop"], tm["rows"] / max(tm["loop"], 1e-9), tm["engine"], tm["write"], tm["reader"]))
        else:
            sys.stderr.write("[cli timing] stream %d of %d: %d blocks, %d rows in %.2f s of the block loop = %.3g rows/s; engine calls (H2D + GPU + D2H) %.2f s, sink (masking, "
                             "counters, formatting, write) %.2f s of which formatting %.2f s and write %.2f s; sink %s; this thread waited %.2f s for the reader and %.2f s for the sink's queue\n"
                             % (i, len(tms), tm["blocks"], tm["rows"], tm["loop"], tm["rows"] / max(tm["loop"], 1e-9), tm["engine"], tm["sink"], tm["format"], tm["write"],
                                "on a worker thread" if tm["overlap"] else "serial", tm["reader"], tm["queue"]))
    now, age = time.time(), float("nan")
    try:                                                   # seconds since this process started (field 22 of /proc/self/stat against the uptime)
        with open("/proc/self/stat") as fh, open("/proc/uptime") as fu:
            st_ = fh.read()
            age = float(fu.read().split()[0]) - int(st_[st_.rindex(")") + 2:].split()[19]) / os.sysconf("SC_CLK_TCK")
    except (OSError, ValueError, IndexError):
        pass
    sys.stderr.write("[cli timing] before the block loop: %.2f s from process start to the model set-up (interpreter, imports, phenotypes, "
                     "structure), %.2f s model set-up (kinship cache / null fit, device context, engine set-up), %.2f s to the first block; "
                     "%.2f s from process start to the end of the loop\n" % (age - (now - t_inputs), t_setup - t_inputs, tms[0]["t0w"] - t_setup, age))
