"""The reference's evaluation / fusion experiment flows without the sacred experiment database
(reference: experiments/evaluation.py:14-41,62-110, experiments/bayes_fusion.py:21-33,146-195,
experiments/dirichlet_fusion.py:19-81, average_mix.py, experiments/training.py, experiments/uncertainty_eval.py:18-52,
experiments/different_evaluation_parameters.py:10-61).

Datasets here are dicts of arrays ({'rgb': [N,H,W,3], 'depth': [N,H,W,1], 'labels': [N,H,W]}) or any iterable of
per-sample dicts (the data contract of base_model.iterate_batches); the reference's `tf.data` readers, the
sacred observers and the experiment-id look-ups of `starting_weights` are out of scope -- `starting_weights` is a
path to an npz in the reference's variable-name schema, a list of such paths, or a {prefix: path} dict.
"""
from copy import deepcopy

import numpy as np

from . import get_model
from .base_model import iterate_batches, score_measures
from .basic_fusion_model import parameter_combinations  # noqa: F401  (the reference's name, defined beside score_grid)
from .bayes_mix import BayesFusion
from .dirichlet_mix import DirichletFusion
from .fusion_comparison import FusionComparison


def import_weights_into_network(net, starting_weights, **kwargs):
    """experiments/evaluation.py:62-110 minus the experiment database: import one or several npz files."""
    if starting_weights is None or starting_weights == '':
        return
    if isinstance(starting_weights, dict):
        starting_weights = list(starting_weights.values())
    if isinstance(starting_weights, (list, tuple)):
        for path in starting_weights:
            net.import_weights(path, warnings=False, **kwargs)
    else:
        net.import_weights(starting_weights, warnings=False, **kwargs)


def split_test_data(testset, test_size=.5, random_state=1):
    """experiments/bayes_fusion.py:21-33: the test set is split in halves, one to measure the experts' statistics on
    (confusion matrices / Dirichlet sufficient statistics) and one to test the fusion on.  Deterministic shuffle like
    sklearn.model_selection.train_test_split(random_state=1)."""
    n = len(next(iter(testset.values())))
    from sklearn.model_selection import train_test_split
    measure_idx, test_idx = train_test_split(np.arange(n), test_size=test_size, random_state=random_state)
    take = lambda idx: {k: np.asarray(v)[idx] for k, v in testset.items()}   # noqa: E731
    return take(measure_idx), take(test_idx)


def evaluate(net, testset, print_results=True, labelinfo=None):
    """experiments/evaluation.py:14-41."""
    measures, confusion_matrix = net.score(testset)
    if print_results:
        print('total accuracy {:.3f} mean F1 {:.3f} IoU {:.3f}'.format(
            measures['total_accuracy'], measures['mean_F1'], measures['mean_IoU']))
        for label in (labelinfo or {}):
            print('{:>15}: {:.2f} precision, {:.2f} recall, {:.2f} IoU'.format(
                labelinfo[label]['name'], measures['precision'][label], measures['recall'][label],
                measures['IoU'][label]))
    return measures, confusion_matrix


def evaluate_groups(net, testset, groups, print_results=True, labelinfo=None):
    """evaluate() per group of images on ONE pass of the network (net.score_groups): {key: (measures, confusion matrix)}.
    groups: one hashable key per image in the order of `testset`, or 'image'."""
    results = net.score_groups(testset, groups)
    if print_results:
        for key, (measures, _) in results.items():
            print('{}: total accuracy {:.3f} mean F1 {:.3f} IoU {:.3f}'.format(
                key, measures['total_accuracy'], measures['mean_F1'], measures['mean_IoU']))
            for label in (labelinfo or {}):
                print('{:>15}: {:.2f} precision, {:.2f} recall, {:.2f} IoU'.format(
                    labelinfo[label]['name'], measures['precision'][label], measures['recall'][label],
                    measures['IoU'][label]))
    return results


def evaluate_agreement(net, testset, print_results=True):
    """evaluate() for the question a fusion raises: where do the experts disagree, and whom does the fusion follow there?
    (net.score_agreement: one pass, the expert-agreement table and its measures.)  Returns (measures, table)."""
    measures, table = net.score_agreement(testset)
    if print_results:
        print('fused accuracy {:.3f} best expert {:.3f} oracle {:.3f}'.format(
            measures['fused_accuracy'], measures['best_expert_accuracy'], measures['oracle_accuracy']))
        for expert, accuracy in measures['expert_accuracy'].items():
            print('{:>15}: {:.3f} accuracy'.format(expert, accuracy))
        print('experts unanimous on {:.3f} of the pixels, fused accuracy where they are not {:.3f}'.format(
            measures['unanimous'], measures['fused_accuracy_on_disagreement']))
        print('rescued {:.4f} lost {:.4f} own-way errors {:.4f}'.format(
            measures['rescued'], measures['lost'], measures['own_way_errors']))
        for expert, share in measures.get('follows', {}).items():
            print('{:>15}: followed on {:.3f} of the disagreements'.format(expert, share))
    return measures, table


def evaluate_calibration(net, testset, temperatures=None, print_results=True):
    """evaluate() for the question a probabilistic fusion raises: can its confidence be believed, and is it more over-confident
    than its experts?  (net.score_calibration: one pass, the reliability tables of the fusion and of every expert.)  Prints
    accuracy, mean confidence, ECE and NLL per expert and for the fusion; with a list of `temperatures` also the temperature of
    least NLL on the fused posterior (net.calibration_search: one more pass) and the measures there.  Returns what
    score_calibration returns, with the calibration_search result as a last entry when temperatures are given."""
    has_experts = bool(getattr(net, 'modalities', None))
    result = net.score_calibration(testset, experts=True) if has_experts else net.score_calibration(testset)
    rows = list(result[2].items()) if has_experts else []
    rows.append(('fusion' if has_experts else 'model', result[:2]))
    search = net.calibration_search(testset, temperatures) if temperatures is not None else None
    if print_results:
        for name, (m, _) in rows:
            print('{:>15}: accuracy {:.3f} confidence {:.3f} ECE {:.4f} NLL {:.4f}'.format(
                name, m['accuracy'], m['mean_confidence'], m['ECE'], m['NLL']))
        if search is not None:
            best = search['measures'][search['temperatures'].index(search['best'])]
            print('best temperature {:g}: ECE {:.4f} NLL {:.4f}'.format(search['best'], best['ECE'], best['NLL']))
    return result + (search,) if search is not None else result


def evaluate_confidence(net, testset, thresholds, temperature=None, print_results=True):
    """What abstaining below a confidence threshold buys: for every threshold the coverage (share of the labelled pixels
    net.predict_confidence(threshold=...) would keep) and the risk (share of wrong labels among them), read off ONE
    net.score_calibration pass (calibration.risk_coverage of its table of 1024 bins) at `temperature` -- by default the one
    fit_temperature stored, else 1.  A threshold is served at the bin edge at or above it, exact for multiples of 1/1024.
    Returns {'thresholds': the edges used, 'coverage', 'risk' (arrays, one entry per threshold), 'area': the area under the
    whole risk-coverage curve, 'measures': the calibration measures}."""
    from .calibration import risk_coverage
    T = float(getattr(net, 'config', {}).get('temperature', 1.0) if temperature is None else temperature)
    measures, table = net.score_calibration(testset, temperature=T)[:2]
    curve = risk_coverage(table)
    NB = len(curve['thresholds'])
    edges = np.minimum(np.ceil(np.asarray(thresholds, np.float64) * NB).astype(np.int64), NB - 1)
    if (edges < 0).any():
        raise ValueError('thresholds lie in [0, 1], got %r' % (thresholds,))
    result = {'thresholds': curve['thresholds'][edges], 'coverage': curve['coverage'][edges], 'risk': curve['risk'][edges],
              'area': curve['area'], 'measures': measures}
    if print_results:
        print('temperature {:g}: accuracy {:.3f} confidence {:.3f} area under risk-coverage {:.4f}'.format(
            T, measures['accuracy'], measures['mean_confidence'], curve['area']))
        for t, c, r in zip(result['thresholds'], result['coverage'], result['risk']):
            print('{:>15}: coverage {:.3f} risk {:.4f}'.format('conf >= %.4g' % t, c, r))
    return result


def evaluate_on_all_sequences(net, testset, sequence_of_image):
    """experiments/evaluation.py:42-55 (evaluate_on_all_synthia_seqs) on one pass instead of one evaluation per sequence:
    sequence_of_image names the sequence of every image of `testset`, in order.  Returns {sequence: measures}."""
    all_measurements = {}
    for sequence, (measurements, _) in evaluate_groups(net, testset, sequence_of_image, print_results=False).items():
        print('Evaluated network on {}: {:.2f} IoU'.format(sequence, measurements['mean_IoU']))
        all_measurements[sequence] = measurements
    return all_measurements


def _resampled_measures(per_image_cms, counts, measure):
    """The measure of every resample: counts int64 [R, N] (how often each image was drawn) times the images' matrices [N, C*C]
    in int64, each sum through score_measures."""
    cms = np.asarray(per_image_cms)
    flat = cms.reshape(len(cms), -1).astype(np.int64)
    sums = (counts @ flat).reshape((len(counts),) + cms.shape[1:])
    return np.array([score_measures(cm)[measure] for cm in sums], np.float64)


def _bootstrap_counts(num_images, num_resamples, seed):
    """int64 [R, N]: per resample, how often each of N images is drawn in N draws with replacement -- one multinomial draw of
    numpy.random.RandomState(seed) per resample, so `seed` fixes them."""
    rng = np.random.RandomState(seed)
    return rng.multinomial(num_images, np.full(num_images, 1.0 / num_images), size=num_resamples).astype(np.int64)


def _percentile_bounds(samples, interval):
    tail = 100.0 * (1.0 - interval) / 2.0
    low, high = np.nanpercentile(samples, [tail, 100.0 - tail])
    return float(low), float(high)


def _as_matrices(per_image_cms):
    """A score_groups result ({key: (measures, matrix)}) or a sequence of [C, C] matrices -> array [N, C, C]."""
    if isinstance(per_image_cms, dict):
        per_image_cms = [cm for _, cm in per_image_cms.values()]
    cms = np.asarray(per_image_cms)
    if cms.ndim != 3 or cms.shape[1] != cms.shape[2] or len(cms) < 1:
        raise ValueError('per-image confusion matrices of shape %s, expected [N, C, C]' % (cms.shape,))
    return cms


def bootstrap_measure(per_image_cms, measure='mean_IoU', num_resamples=1000, seed=0, interval=0.95):
    """Bootstrap interval of a scalar measure of score() over the images: per resample N images are drawn with replacement,
    their confusion matrices summed and the measure taken from the sum (score_measures).  per_image_cms: [N, C, C] (or what
    score_groups(..., 'image') returns).  Returns {'value': the measure of all images, 'low', 'high': the percentile bounds of
    `interval`, 'samples': float64 [num_resamples]}.  `seed` fixes the draws: the same seed gives the same samples."""
    cms = _as_matrices(per_image_cms)
    samples = _resampled_measures(cms, _bootstrap_counts(len(cms), num_resamples, seed), measure)
    low, high = _percentile_bounds(samples, interval)
    return {'value': float(score_measures(cms.sum(0))[measure]), 'low': low, 'high': high, 'samples': samples}


def paired_bootstrap(per_image_cms_a, per_image_cms_b, measure='mean_IoU', num_resamples=1000, seed=0, interval=0.95):
    """bootstrap_measure of the difference a - b of two methods scored on the SAME images (two rows of
    FusionComparison.score_all_groups(..., 'image')): every resample draws the same images for both.  Returns {'value', 'low',
    'high', 'samples'} of the difference and 'fraction_a_better': the share of resamples with a > b.  `seed` fixes the draws."""
    a, b = _as_matrices(per_image_cms_a), _as_matrices(per_image_cms_b)
    if a.shape != b.shape:
        raise ValueError('paired matrices of shapes %s and %s' % (a.shape, b.shape))
    counts = _bootstrap_counts(len(a), num_resamples, seed)
    samples_a, samples_b = _resampled_measures(a, counts, measure), _resampled_measures(b, counts, measure)
    samples = samples_a - samples_b
    low, high = _percentile_bounds(samples, interval)
    value = float(score_measures(a.sum(0))[measure] - score_measures(b.sum(0))[measure])
    return {'value': value, 'low': low, 'high': high, 'samples': samples,
            'fraction_a_better': float(np.mean(samples_a > samples_b))}


def train_and_evaluate(modelname, net_config, data_description, trainset, testset, num_iterations, starting_weights=None,
                       validation_set=None, output_dir=None):
    """experiments/training.py: build the model, optionally warm-start, fit, export the weights, evaluate."""
    info = {}
    with get_model(modelname)(data_description=data_description, output_dir=output_dir, **net_config) as net:
        import_weights_into_network(net, starting_weights)
        net.fit(trainset, num_iterations, output=False, validation_dataset=validation_set)
        info['weights'] = net.export_weights() if output_dir else None
        info['measurements'], info['confusion_matrix'] = evaluate(net, testset, print_results=False)
    return info


def fit_and_evaluate_bayes_fusion(net_config, data_description, measure_set, test_set, starting_weights):
    """experiments/bayes_fusion.py:146-195: score every expert on the measurement set (its confusion matrix feeds the
    fusion) and on the test set, then score the Bayes fusion on the test set.
    net_config: expert_model, prefixes, num_channels, num_units, class_prior, ...; starting_weights: {prefix: npz}."""
    info = {'measurements': {}}
    model = get_model(net_config['expert_model'])
    confusion_matrices = {}
    for expert in net_config['num_channels']:
        model_config = deepcopy(net_config)
        prefix = net_config['prefixes'][expert]
        for key in ('prefixes', 'num_channels', 'expert_model', 'class_prior'):
            model_config.pop(key, None)
        model_config.setdefault('batch_normalization', False)
        with model(prefix, data_description, expert, **model_config) as net:
            import_weights_into_network(net, starting_weights[prefix] if isinstance(starting_weights, dict)
                                        else starting_weights)
            _, conf_mat = net.score(measure_set)
            confusion_matrices[expert] = conf_mat
            info['measurements'][expert], _ = net.score(test_set)
    info['confusion_matrices'] = confusion_matrices
    with BayesFusion(data_description=data_description, confusion_matrices=confusion_matrices, **net_config) as net:
        import_weights_into_network(net, starting_weights)
        info['measurements']['fusion'], info['confusion_matrix'] = net.score(test_set)
    return info


def collect_predictions(net, measure_set, test_set, save_to):
    """experiments/ibcc_fusion.py:18-42: every expert's label maps on both halves and the ground truth, written as
    `predictions.npz` under `save_to` -- the file an external IBCC reads.  Keys: measure_<modality>, test_<modality> (int64
    [N,H,W]), measure_gt, test_gt (the sets' own labels).  net: a fusion model (its experts are run once per half, through its
    `expert_outputs`, with the fused head off so that they are materialised).  Returns the file's path."""
    import os
    predictions = {}
    fused_head = net.config.get('fused_head', True)
    net.config['fused_head'] = False
    try:
        for part, data in (('measure', measure_set), ('test', test_set)):
            maps = {m: [] for m in net.modalities}
            for batch in iterate_batches(data, net.config['batchsize']):
                net.predict(batch)
                for m in net.modalities:
                    label = net.expert_outputs[m]['classification']
                    maps[m].append(np.asarray(label.cpu() if hasattr(label, 'cpu') else label).astype(np.int64))
            for m in net.modalities:
                predictions['%s_%s' % (part, m)] = np.concatenate(maps[m])
            predictions['%s_gt' % part] = np.asarray(data['labels']) if isinstance(data, dict) else \
                np.stack([np.asarray(sample['labels']) for sample in data])
    finally:
        net.config['fused_head'] = fused_head
    os.makedirs(save_to, exist_ok=True)
    path = os.path.join(save_to, 'predictions.npz')
    np.savez_compressed(path, **predictions)
    return path


def fit_and_evaluate_ibcc(net_config, data_description, measure_set, test_set, starting_weights, adapt_set=None):
    """The IBCC counterpart of fit_and_evaluate_bayes_fusion: every expert's confusion matrix from ONE pass of the experts
    over the measurement set (IbccFusion.measure), then the fusion with those priors scored on the test set twice -- by its
    priors alone, and after adapt() on `adapt_set` (default: the test set's images; its labels are never read).  Returns {'confusion_matrices', 'prior': (measures, cm), 'adapted': (measures, cm), 'ibcc': the
    adaptation's ibcc.IbccResult}."""
    from .ibcc_mix import IbccFusion
    info = {}
    C = data_description[2]
    flat = {m: np.ones((C, C)) for m in net_config['prefixes']}          # flat priors until the experts are measured
    with IbccFusion(data_description=data_description, confusion_matrices=flat, **net_config) as net:
        import_weights_into_network(net, starting_weights)
        info['confusion_matrices'] = net.measure(measure_set)
        info['prior'] = net.score(test_set)
        info['ibcc'] = net.adapt(test_set if adapt_set is None else adapt_set)
        info['adapted'] = net.score(test_set)
    return info


def fit_and_evaluate_dirichlet_fusion(net_config, data_description, measure_set, test_set, starting_weights):
    """experiments/dirichlet_fusion.py:58-81: fit the Dirichlet parameters on the measurement set, re-import the
    weights, score on the test set."""
    info = {}
    with DirichletFusion(data_description=data_description, **net_config) as net:
        import_weights_into_network(net, starting_weights)
        info['dirichlet_params'] = net.fit(measure_set)
        import_weights_into_network(net, starting_weights)
        info['measurements'], info['confusion_matrix'] = net.score(test_set)
    return info


def fit_and_evaluate_all_fusions(net_config, data_description, measure_set, test_set, starting_weights):
    """The table of the two flows above and of an AverageFusion on the same split, from ONE pass of the experts over each half
    (fusion_comparison.FusionComparison): measure every expert's confusion matrix and the Dirichlet statistics on the
    measurement set, then score every expert alone and the Bayes, Dirichlet and average fusion on the test set.
    net_config: a Bayes-fusion config (expert_model, prefixes, num_channels, num_units, class_prior, ...) plus sigma, delta,
    beta.  Returns {'measurements': {modality: ..., 'bayes_fusion': ..., 'dirichlet_fusion': ..., 'average_fusion': ...},
    'confusion_matrix': the same keys, 'confusion_matrices': {modality: [C,C]}, 'dirichlet_params': {modality: [C,C],
    'class_counts': [C]}} -- the last two are what BayesFusion and DirichletFusion take as measurements."""
    info = {'measurements': {}, 'confusion_matrix': {}}
    with FusionComparison(data_description=data_description, **net_config) as net:
        import_weights_into_network(net, starting_weights)
        info.update(net.fit(measure_set))
        for name, (measures, confusion_matrix) in net.score_all(test_set).items():
            info['measurements'][name], info['confusion_matrix'][name] = measures, confusion_matrix
    return info


def evaluate_uncertainty(net, data, metric, benchmark='misclassification', print_results=True, ood_data=None):
    """experiments/uncertainty_eval.py:18-32: ROC and AUROC of one uncertainty metric of `net` (an UncertaintyModel) as a
    detector of its misclassified pixels, or (benchmark 'out_of_distribution') of the pixels of `ood_data` among those of
    `data` (the reference's base class drew the foreign set from the dataset itself; here it is an argument)."""
    if benchmark == 'misclassification':
        fpr, tpr, auroc, thresholds = net.misclassification_detection_score(data, metric)
    elif benchmark == 'out_of_distribution':
        if ood_data is None:
            raise ValueError("benchmark 'out_of_distribution' needs ood_data")
        fpr, tpr, auroc, thresholds = net.out_of_distribution_detection_score(data, metric, ood_data)
    else:
        raise ValueError('unknown benchmark %r' % (benchmark,))
    if print_results:
        print('Uncertainty Benchmark "{}" of {} on {} with {} metric'.format(benchmark, net.name, type(data).__name__, metric))
        print('AUROC {:.3f}'.format(auroc))
    return {'TPR': tpr, 'FPR': fpr, 'AUROC': auroc, 'thresholds': thresholds}


def measure_metrics(net, data, metrics):
    """experiments/uncertainty_eval.py:35-39 (its label_flip / mean_diff / prob_distribution parts belong to ambiguous-label
    training, which is out of scope): {'nll', 'class_counts', and per metric its value_distribution}."""
    nll, class_count = net.nll_score(data)
    ret = {'nll': nll, 'class_counts': class_count}
    for metric in metrics:
        ret[metric] = net.value_distribution(data, metric)
    return ret


def evaluate_fusion_uncertainty(net, testset, ood_set=None, print_results=True):
    """evaluate_uncertainty for the question a modular fusion exists to answer: does the fused posterior know when it is
    wrong better than either expert does?  ONE pass per data set (net.uncertainty_tables with every expert's own tables):
    per expert and for the fusion the AUROC of every metric of net.uncertainty_metrics as a detector of that row's own
    misclassified pixels, with `ood_set` the same as a detector of its pixels (all of them) among the labelled pixels of
    `testset`, and the mean NLL over the labelled pixels.  Returns {row: {'misclassification': {metric: AUROC},
    'out_of_distribution': {metric: AUROC} (with ood_set), 'nll': float}}, the fusion under 'fusion'."""
    from .uncertainty_model import roc_from_histogram
    inside = net.uncertainty_tables(testset, experts=True)
    outside = net.uncertainty_tables(ood_set, experts=True, fixed_row=1) if ood_set is not None else None
    rows = [(name, t, outside['experts'][name] if outside else None) for name, t in inside['experts'].items()]
    rows.append(('fusion', inside, outside))
    result = {}
    for name, t, foreign in rows:
        counts = int(t['counts'].sum())
        r = result[name] = {'misclassification': {m: roc_from_histogram(t['hist'][i], t['edges'])[2]
                                                  for i, m in enumerate(t['metrics'])},
                            'nll': float(t['nll_sum'].sum() / counts) if counts else float('nan')}
        if foreign is not None:
            r['out_of_distribution'] = {m: roc_from_histogram(np.stack([t['hist'][i].sum(0), foreign['hist'][i][1]]), t['edges'])[2]
                                        for i, m in enumerate(t['metrics'])}
        if print_results:
            line = '{:>15}: NLL {:.4f} misclassification AUROC'.format(name, r['nll'])
            line += ''.join(' {} {:.3f}'.format(m, a) for m, a in r['misclassification'].items())
            if foreign is not None:
                line += ' out-of-distribution AUROC' + ''.join(' {} {:.3f}'.format(m, a) for m, a in r['out_of_distribution'].items())
            print(line)
    return result


def _collect(results, values):
    """Append every leaf of the (nested) dict `values` to the list under the same keys of `results`."""
    for key, value in values.items():
        if isinstance(value, dict):
            _collect(results.setdefault(key, {}), value)
        else:
            results.setdefault(key, []).append(value)


def grid_search(evaluation, search_parameters, net_config):
    """experiments/different_evaluation_parameters.py:27-61: evaluation(config) -> (nested) dict of measurements, called once
    per combination of `search_parameters` (lists of values; the first key varies slowest) on top of `net_config`.  Returns one
    dict in which every config key and every measurement is a list over the grid points, nested measurement dicts merged key
    by key.  One model per grid point: for the parameters of the fusion itself, grid_search_fusion takes one pass."""
    results = {}
    for config in parameter_combinations(search_parameters, net_config):
        for key in config:                       # a config value is one entry, a dict among them
            results.setdefault(key, []).append(config[key])
        _collect(results, evaluation(config))
    return results


def grid_search_fusion(net, testset, search_parameters):
    """grid_search's result for a fusion model's own parameters (DirichletFusion: sigma, class_prior, delta, beta;
    BayesFusion: class_prior) from ONE pass of the experts over `testset` (net.score_grid): the config keys of `net` and the
    measures of score() as lists over the grid points."""
    results = {}
    for config, measures, _ in net.score_grid(testset, search_parameters):
        for key in config:
            results.setdefault(key, []).append(config[key])
        _collect(results, measures)
    return results
