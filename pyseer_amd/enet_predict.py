"""Predict phenotypes from a saved elastic-net model (pyseer/enet_predict.py) with the sum on the device.

    python -m pyseer_amd.enet_predict MODEL SAMPLES (--kmers F | --vcf F | --pres F | --load-packed F) [--covariates F --use-covariates ...]

MODEL is what `python -m pyseer_amd --wg enet --save-enet-model` wrote (text), or the reference's --save-model pickle.  The prediction of a
sample is the intercept, plus its covariates times their slopes, plus the slope of every model variant it carries, added in the order of the
input (k_enet_predict keeps that order: the printed numbers are the reference's, digit for digit).  K-mers and the packed cache come as raw
blocks from the native reader and are matched to the model by name in the library (sh_nameset_*); a VCF comes through the native VCF
reader and an Rtab (--pres) through the native Rtab reader; --burden and --python-reader go line by line through read_variant.  All routes
print the same bytes.
"""
import argparse
import collections
import sys

import numpy as np

VCF_PACKED_MESSAGE = '--gpus and the packed cache (--save-packed / --load-packed / --packed-cache / --packed-part) are not available with --vcf\n'


def get_options(argv=None):
    parser = argparse.ArgumentParser(description='Predict phenotypes using a fitted elastic net model', prog='python -m pyseer_amd.enet_predict')
    parser.add_argument('model', help='Fitted model: the text file of --save-enet-model, or a --save-model pickle of the reference')
    parser.add_argument('samples', help='File with samples to predict')
    parser.add_argument('--threshold', help='Threshold to pick binary predictions', type=float, default=0.5)
    parser.add_argument('--lineage-clusters', help='Custom clusters to use as lineages to report stratified accuracy')
    parser.add_argument('--true-values', help='Pheno file with known phenotypes to calculate accuracy', default=None)
    parser.add_argument('--ignore-missing', help='Treat missing values as REF/0 rather than using the mean AF', action='store_true', default=False)
    variants = parser.add_argument_group('Variants')
    group = variants.add_mutually_exclusive_group()
    group.add_argument('--kmers', default=None, help='Kmers file')
    group.add_argument('--vcf', default=None, help='VCF file. Will filter any non \'PASS\' sites')
    group.add_argument('--pres', default=None, help='Presence/absence .Rtab matrix as produced by roary and piggy')
    variants.add_argument('--burden', help='VCF regions to group variants by for burden testing (requires --vcf)')
    variants.add_argument('--uncompressed', action='store_true', default=False, help='Uncompressed kmers file [Default: gzipped]')
    covariates = parser.add_argument_group('Covariates')
    covariates.add_argument('--covariates', default=None, help='User-defined covariates file (tab-delimited, first column contains sample names)')
    covariates.add_argument('--use-covariates', default=None, nargs='*', help='Covariates to use. Format is "2 3q 4" (q for quantitative)')
    ot = parser.add_argument_group('Other')
    ot.add_argument('--gpu', type=int, default=0, help='GPU index [Default: 0]')
    ot.add_argument('--python-reader', action='store_true', default=False, help='Parse k-mer, VCF and Rtab files with the Python reader instead of the native one')
    ot.add_argument('--load-packed', default=None, help='Read k-mers from a packed cache written by an earlier run over the same samples instead of --kmers')
    ot.add_argument('--block_size', type=int, default=3000, help='Number of variants parsed at a time')
    options = parser.parse_args(argv)
    if not (options.kmers or options.vcf or options.pres or options.load_packed):
        parser.error('one of the arguments --kmers --vcf --pres (or --load-packed) is required')
    return options


def _die(msg):
    sys.stderr.write(msg)
    sys.exit(1)


class _Model(object):
    """The variants of the model (what is left once the intercept and the loaded covariates are taken out), in the model's order."""

    def __init__(self, entries):
        self.names = list(entries.keys())
        self.af = np.array([entries[k][0] for k in self.names], dtype=float)
        self.beta = np.array([entries[k][1] for k in self.names], dtype=float)
        self.flip = self.af > 0.5                                     # the model is fitted to minor-allele coded variants (enet_predict.py:177)
        self.met = np.zeros(len(self.names), dtype=bool)


def _kmer_blocks(options, samples_index):
    from .input import check_kmers_gzipped, check_packed_cache, iter_packed_blocks_cached, iter_packed_blocks_native
    block_size = max(options.block_size, 1 << 18)
    if options.load_packed:
        try:
            check_packed_cache(samples_index, options.load_packed)
        except (IOError, OSError, ValueError) as e:
            _die("%s\n" % e)
        return iter_packed_blocks_cached(samples_index, options.load_packed, 0.0, 1.0, block_size, raw=True, device=None, say_empty=False)
    if not options.uncompressed:
        check_kmers_gzipped([options.kmers])
    return iter_packed_blocks_native(samples_index, options.kmers, 0.0, 1.0, block_size, raw=True, say_empty=False)


def _predict_kmer_blocks(blocks, model, predictor):
    """Raw blocks of the native reader or the packed cache: the names are matched in the library, only the model's rows leave the host."""
    from .enet import NameSet
    names = NameSet(model.names)
    try:
        for blk in blocks:
            rows, which = names.match(blk.blob, blk.off)
            if rows.size:
                model.met[which] = True
                for r in rows[blk.counts[rows] == 0]:                 # (read_variant says so for every line it parses)
                    sys.stderr.write("No observations of " + bytes(blk.blob[blk.off[r]:blk.off[r + 1]]).decode() + " in selected samples\n")
                use = model.beta[which] != 0                          # (`if pred_beta != 0`: such an entry is met, retired and adds nothing)
                predictor.add(blk.bits, rows[use], model.beta[which[use]], model.flip[which[use]])
            if blk.release is not None:
                blk.release()
            if names.left == 0:                                       # the reference's loop ends on an empty dict
                break
    finally:
        names.close()


def _predict_vcf_native(options, samples, engine, model, predictor):
    """Records of the native VCF reader: a record that is kept (one ALT, a passing FILTER) is matched by name; one with several ALTs is only
    reported when the model names it (read_vcf_var looks at nothing else of a record outside the keep_list, pyseer/input.py:473-478)."""
    from .enet import NameSet, _take_names
    from .input import NativeVcfReader, VCF_KEPT, VCF_MULTI
    wanted = set(model.names)
    names = NameSet(model.names)
    reader = NativeVcfReader(options.vcf, samples, engine, max(options.block_size, 1))
    try:
        for blk in reader.raw_blocks():
            blob, off, skip = blk["blob"], blk["off"], blk["skip"]
            kept = np.nonzero(skip == VCF_KEPT)[0]
            sub_blob, sub_off = _take_names(blob, off, kept)
            sub_rows, which = names.match(sub_blob, sub_off)
            rows = kept[sub_rows]
            model.met[which] = True
            says = [(int(r), "No observations of " + blob[off[r]:off[r + 1]].decode() + " in selected samples\n")
                    for r in rows[(blk["n_present"][rows] + blk["n_missing"][rows]) == 0]]
            for r in np.nonzero(skip == VCF_MULTI)[0]:
                if blob[off[r]:off[r + 1]].decode().replace(',', '_') in wanted:
                    says.append((int(r), "Multiple alleles at %s_%d. Skipping\n" % (reader.contig(blk["contig"][r]), int(blk["pos"][r]))))
            for _, text in sorted(says):
                sys.stderr.write(text)
            use = model.beta[which] != 0
            sel = rows[use]
            if sel.size:
                miss = blk["missing"] if np.any(blk["n_missing"][sel] > 0) else None
                predictor.add(blk["present"], sel, model.beta[which[use]], model.flip[which[use]], missing=miss)
            if names.left == 0:
                break
    finally:
        reader.close()
        names.close()


def _predict_rtab_native(options, samples, engine, model, predictor):
    """Lines of the native Rtab reader, matched by name.  Only a matched line is looked at: one that is malformed raises read_variant's
    ValueError, after the matched lines before it have said what read_variant says of them; a malformed line the model does not name is passed
    over, as read_variant returns before its checks for a name outside the keep_list.  Returns False, with nothing read, for a header that
    names a sample twice (the caller reads line by line)."""
    from .enet import NameSet
    from .input import NativeRtabReader, RtabDuplicateSample, RTAB_ERRORS
    try:
        reader = NativeRtabReader(options.pres, samples, engine, max(options.block_size, 1))
    except RtabDuplicateSample:
        return False
    names = NameSet(model.names)
    try:
        for blk in reader.raw_blocks():
            blob, off = blk["blob"], blk["off"]
            rows, which = names.match(blob, off)
            bad = np.nonzero(blk["status"][rows])[0]
            upto = int(bad[0]) if bad.size else rows.size                 # matched lines before the first malformed one
            for r in rows[:upto][(blk["n_present"][rows[:upto]] + blk["n_missing"][rows[:upto]]) == 0]:
                sys.stderr.write("No observations of " + blob[off[r]:off[r + 1]].decode() + " in selected samples\n")
            if bad.size:
                raise ValueError(RTAB_ERRORS[int(blk["status"][rows[upto]])])
            model.met[which] = True
            use = model.beta[which] != 0
            sel = rows[use]
            if sel.size:
                miss = blk["missing"] if np.any(blk["n_missing"][sel] > 0) else None
                predictor.add(blk["present"], sel, model.beta[which[use]], model.flip[which[use]], missing=miss)
            if names.left == 0:
                break
    finally:
        reader.close()
        names.close()
    return True


def _predict_lines(options, p, model, predictor, var_type, var_file):
    """--burden and --python-reader (and an Rtab whose header names a sample twice): the reference's loop over read_variant (enet_predict.py:159-179), its rows packed in blocks."""
    from .input import open_variant_file, read_variant
    from .packing import row_bytes_for
    n, rb = len(p), row_bytes_for(len(p))
    burden_regions = collections.deque([])
    infile, sample_order = open_variant_file(var_type, var_file, options.burden, burden_regions, options.uncompressed)
    all_strains = set(p.index)
    left = collections.OrderedDict((name, i) for i, name in enumerate(model.names))
    pres, miss, which = [], [], []

    def flush():
        if not which:
            return
        def pack(rows):
            out = np.zeros((len(rows), rb), dtype=np.uint8)
            pk = np.packbits(np.array(rows, dtype=bool).reshape(len(rows), n), axis=1, bitorder="little")
            out[:, :pk.shape[1]] = pk
            return out
        w = np.array(which)
        has_missing = any(m.any() for m in miss)
        predictor.add(pack(pres), np.arange(len(which)), model.beta[w], model.flip[w], missing=pack(miss) if has_missing else None)
        del pres[:], miss[:], which[:]
    while True:
        eof, k, var_name, kstrains, nkstrains, af, missing = read_variant(infile, p, var_type, bool(options.burden), burden_regions,
                                                                          options.uncompressed, all_strains, sample_order, keep_list=left.keys())
        if eof or len(left) == 0:
            break
        i = left.pop(var_name, None)
        if i is None:
            continue
        model.met[i] = True
        if model.beta[i] != 0:
            k = np.asarray(k, dtype=float)
            pres.append(k == 1); miss.append(np.isnan(k)); which.append(i)
            if len(which) >= 4096:
                flush()
    flush()


def _summary(options, samples, continuous, link, classes, fold_ids, lineage_dict):
    """enet_predict.py:212-239.  Every figure is taken over the samples that have a true value, aligned by name (the reference hands
    write_lineage_predictions the true values of those samples beside the predictions of all of them)."""
    from .enet import _r2, write_lineage_predictions
    from .input import load_phenotypes
    y_all = load_phenotypes(options.true_values, None)
    have = [i for i, s in enumerate(samples) if s in y_all.index]
    y_true = y_all.loc[[samples[i] for i in have]].values.astype(float)
    pred = (link if continuous else classes)[have]
    sys.stderr.write("Overall prediction accuracy\n")
    sys.stderr.write("R2: " + str(_r2(y_true, pred)) + "\n")
    if not continuous:
        for label, t, q in (("tn", 0, 0), ("fp", 0, 1), ("fn", 1, 0), ("tp", 1, 1)):
            sys.stderr.write(label + ": " + str(int(np.sum((y_true == t) & (pred == q)))) + "\n")
    if fold_ids is not None:
        sys.stderr.write("Predictions within each lineage\n")
        write_lineage_predictions(y_true, pred, fold_ids[have], lineage_dict, continuous, sys.stderr)


def main(argv=None):
    options = get_options(argv)
    if options.burden and not options.vcf:
        _die('Burden test can only be performed with VCF input\n')
    if options.vcf and options.load_packed:
        _die(VCF_PACKED_MESSAGE)
    if options.load_packed and (options.pres or options.python_reader):
        _die('The packed cache holds k-mer lines and is read by the native reader: --load-packed cannot be combined with --pres or --python-reader\n')
    import pandas as pd
    from scipy.special import expit
    from . import _abi
    from .enet import EnetPredictor, read_model
    from .engine import Engine
    from .input import load_covariates, load_lineage
    try:
        model_dict, continuous = read_model(options.model)
    except (IOError, OSError, ValueError) as e:
        _die("Cannot read the model %s: %s\n" % (options.model, e))
    try:
        intercept = model_dict.pop('intercept')[1]
    except KeyError:
        sys.stderr.write("Intercept not found in model\n")
        intercept = 0
    with open(options.samples, 'r') as sample_file:
        samples = [line.rstrip() for line in sample_file]
    p = pd.DataFrame(data=np.full(len(samples), intercept), index=samples, columns=['prediction'])
    start = np.array(p.values, dtype=np.float64).reshape(-1)
    if options.covariates is not None:
        cov = load_covariates(options.covariates, options.use_covariates, p)
        if cov is None:
            sys.exit(1)
        for covariate in cov:
            pred_beta = model_dict.pop(str(covariate), (0, 0))
            if pred_beta[1] != 0:
                start += (cov[covariate] * pred_beta[1]).values
    if options.lineage_clusters:
        lineage_clusters, lineage_dict = load_lineage(options.lineage_clusters, p)
        fold_ids = np.where(lineage_clusters == 1)[1]
    else:
        lineage_dict = fold_ids = None
    model = _Model(model_dict)
    var_type, var_file = ("kmers", options.kmers) if (options.kmers or options.load_packed) else (("vcf", options.vcf) if options.vcf else ("Rtab", options.pres))
    native_kmers = var_type == "kmers" and not options.python_reader
    blocks = _kmer_blocks(options, p) if native_kmers else None      # (the input is checked before the device is opened)
    if __name__ == "__main__":
        _abi.TORCH_FIRST = False                                      # (nothing here reaches torch: _abi.load)
    engine = Engine(len(samples), device=options.gpu)
    predictor = EnetPredictor(engine, start)
    try:
        sys.stderr.write("Reading variants from input\n")
        if native_kmers:
            _predict_kmer_blocks(blocks, model, predictor)
        elif var_type == "vcf" and not options.python_reader and not options.burden:
            _predict_vcf_native(options, samples, engine, model, predictor)
        elif var_type == "Rtab" and not options.python_reader and _predict_rtab_native(options, samples, engine, model, predictor):
            pass
        else:
            _predict_lines(options, p, model, predictor, var_type, var_file)
        link = predictor.finish()
    finally:
        predictor.close()
        engine.close()
    # what the input did not hold is imputed at the model's own frequency: af * beta, also for an entry coded by its absences (the
    # reference's literal rule, enet_predict.py:182-185)
    for i in np.nonzero(~model.met)[0]:
        sys.stderr.write("Could not find covariate/variant " + model.names[i] + " in input file\n")
        if not options.ignore_missing:
            link += model.af[i] * model.beta[i]
    out = sys.stdout
    if continuous:
        classes = None
        out.write("\t".join(['Sample', 'Link', 'Prediction']) + "\n")
        for name, x in zip(samples, link):
            out.write("\t".join([name, str(float(x)), str(float(x))]) + "\n")
    else:
        prob = expit(link)
        classes = np.zeros(link.shape[0])
        classes[np.where(prob > options.threshold)[0]] = 1
        out.write("\t".join(['Sample', 'Prediction', 'Link', 'Probability']) + "\n")
        for i, name in enumerate(samples):
            out.write("\t".join([name, str(classes[i]), str(float(link[i])), str(float(prob[i]))]) + "\n")
    out.flush()
    if options.true_values:
        _summary(options, samples, continuous, link, classes, fold_ids, lineage_dict)


if __name__ == "__main__":
    main()
