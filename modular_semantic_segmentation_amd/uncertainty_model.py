"""Uncertainty benchmarks (reference: xview/models/uncertainty_model.py, which the reference does not ship; the contract is its
call sites, experiments/uncertainty_eval.py:18-52,62-88, and custom_layers.py:239-248 for the temperature).

How good is a per-pixel uncertainty map?  Misclassification detection asks whether it is larger where the label is wrong,
out-of-distribution detection whether it is larger on foreign data (both: ROC curve and AUROC of the map as a detector); the
NLL asks how much probability the mean prediction left for the true class; a temperature search repeats all of it with the
logits divided by a temperature.

Nothing per pixel leaves the device.  The kernels (xv_mc_uncertainty_score_fwd for the Bayesian FCN: the uncertainty head with
the tables where its map stores were; xv_uncertainty_stats for any model's materialised maps; xv_confidence_stats and
xv_fused_head_multi_confidence_stats_fwd for the confidence of every other model's and every fusion's class scores:
confidence_tables_reference states what they count) reduce a data set to

    hist   int64 [metric][row][bin]   row = (prediction != label) over the pixels with a valid label, or a row fixed by the
                                      caller (in-distribution data 0, out-of-distribution data 1) over every pixel
    nll    float64 [C]                -sum ln(clip(mean[label], 1e-10, 1)) over the pixels of each ground-truth class
    counts int64 [C]

and the ROC is computed here from two histogram rows.  A value's bin is a function of its float32 BIT PATTERN (bin_index):
`mantissa_bits` M and `octaves` give octaves << M log-spaced bins of 2^-M relative width covering [2^(1-octaves), 2), with
everything below in bin 0 and everything above (and NaN) in the top bin -- exact, the same in numpy and in the kernels, so
device tables are tested integer for integer.  Binning loses only the order of pairs that share a bin: the AUROC is within
auroc_tie_bound(hist) of the exact rank statistic."""
import numpy as np
import torch

from . import ops

METRICS = ops.UNCERTAINTY_METRICS
CONFIDENCE_METRICS = ops.CONFIDENCE_METRICS


def _check_bins(mantissa_bits, octaves):
    m, o = int(mantissa_bits), int(octaves)
    if not (3 <= m <= 8 and 8 <= o <= 32):
        raise ValueError('mantissa_bits must lie in 3..8 and octaves in 8..32')
    return m, o


def bin_index(values, mantissa_bits=5, octaves=24):
    """Histogram bin (int64, the shape of `values`) of float32 values: v <= 0 and -0.0 -> 0, NaN -> the top bin, else
    (bits(v) >> (23 - M)) - ((128 - octaves) << M) clamped to [0, (octaves << M) - 1] (xv_unc_bin, csrc/xv_common.h)."""
    m, o = _check_bins(mantissa_bits, octaves)
    v = np.ascontiguousarray(values, np.float32)
    top = (o << m) - 1
    key = (v.view(np.uint32) >> np.uint32(23 - m)).astype(np.int64) - ((128 - o) << m)
    key = np.clip(key, 0, top)
    key[~(v > 0)] = 0
    key[np.isnan(v)] = top
    return key


def bin_edges(mantissa_bits=5, octaves=24):
    """float64 [bins + 1]: bin b holds edges[b] <= v < edges[b + 1]; edges[0] = 0 (bin 0 also takes every negative value),
    edges[bins] = inf (the top bin also takes NaN)."""
    m, o = _check_bins(mantissa_bits, octaves)
    bins = o << m
    bits = ((np.arange(1, bins, dtype=np.int64) + ((128 - o) << m)) << (23 - m)).astype(np.uint32)
    return np.concatenate([[0.0], bits.view(np.float32).astype(np.float64), [np.inf]])


def _rows(hist):
    h = np.asarray(hist)
    if h.ndim != 2 or h.shape[0] != 2:
        raise ValueError('a histogram of shape [2, bins]')
    return [int(x) for x in h[0]], [int(x) for x in h[1]]          # Python integers: products of counts pass 2^63


def roc_from_histogram(hist, edges=None):
    """(fpr, tpr, auroc, thresholds) of the detector `value >= threshold` from hist [2][bins] (row 0 negatives, row 1
    positives).  Thresholds are inf (nothing detected: the point (0, 0)) and then the bins' lower edges in descending order,
    so fpr / tpr (float64 [bins + 1], from cumulative counts) are monotone and end at (1, 1).  AUROC by the trapezoid rule,
    which gives the pairs that share a bin one half; summed in integers -- sum_b neg_b (2 pos_above_b + pos_b) over 2 P N -- so
    separable rows give exactly 1 and identical rows exactly 0.5.  NaN when a row is empty."""
    neg, pos = _rows(hist)
    bins = len(neg)
    if edges is None:
        edges = np.arange(bins + 1, dtype=np.float64)
        edges[-1] = np.inf
    N, P = sum(neg), sum(pos)
    cn = np.concatenate([[0], np.cumsum(np.asarray(hist)[0][::-1], dtype=np.int64)])
    cp = np.concatenate([[0], np.cumsum(np.asarray(hist)[1][::-1], dtype=np.int64)])
    with np.errstate(divide='ignore', invalid='ignore'):
        fpr, tpr = cn / np.float64(N), cp / np.float64(P)
    thresholds = np.concatenate([[np.inf], np.asarray(edges, np.float64)[bins - 1::-1]])
    if N == 0 or P == 0:
        return fpr, tpr, float('nan'), thresholds
    area2, above = 0, 0
    for b in range(bins - 1, -1, -1):
        area2 += neg[b] * (2 * above + pos[b])
        above += pos[b]
    return fpr, tpr, area2 / (2 * P * N), thresholds


def auroc_tie_bound(hist):
    """|AUROC of the histogram - exact rank AUROC (ties one half)| <= 0.5 sum_b pos_b neg_b / (P N): binning is monotone, so
    only a positive and a negative that share a bin can be ordered differently, and each such pair moves the statistic by at
    most one half of 1 / (P N)."""
    neg, pos = _rows(hist)
    N, P = sum(neg), sum(pos)
    if N == 0 or P == 0:
        return float('nan')
    return sum(p * n for p, n in zip(pos, neg)) / (2 * P * N)


def confidence_tables_reference(maps, win, labels, nll_pixel=None, num_classes=None, fixed_row=-1, mantissa_bits=5,
                                octaves=24, tables=None):
    """THE DEFINITION of what ops.confidence_stats / ops.fused_head_multi_confidence_stats count, on the host: from the maps
    ops.confidence_map writes ({'entropy', 'confidence', 'margin'}: float32 arrays of one shape) the three
    ops.CONFIDENCE_METRICS -- entropy, float32(1) - confidence, float32(1) - margin, one IEEE float32 operation each -- binned
    by bin_index into hist int64 [3, 2, bins]: row = (win != labels) over the pixels with 0 <= label < C (`win`: the label
    map), or `fixed_row` (0 / 1) for every pixel, void ones included.  With labels, over the valid pixels, nll float64 [C] +=
    nll_pixel (float32 per pixel; None: nothing is added) and counts int64 [C] += 1 per ground-truth class.  Adds into
    `tables` ({'hist', 'nll', 'counts'}) where given; returns them."""
    m, o = _check_bins(mantissa_bits, octaves)
    bins = o << m
    one = np.float32(1.0)
    values = (np.asarray(maps['entropy'], np.float32).ravel(), one - np.asarray(maps['confidence'], np.float32).ravel(),
              one - np.asarray(maps['margin'], np.float32).ravel())
    npix = values[0].size
    if fixed_row not in (-1, 0, 1) or (fixed_row < 0 and labels is None):
        raise ValueError('fixed_row is -1 (rows by correctness: labels needed), 0 or 1')
    if tables is None:
        if num_classes is None:
            raise ValueError('num_classes is needed to make the tables')
        tables = {'hist': np.zeros((3, 2, bins), np.int64), 'nll': np.zeros(num_classes, np.float64),
                  'counts': np.zeros(num_classes, np.int64)}
    C = len(tables['counts'])
    if tables['hist'].shape != (3, 2, bins):
        raise ValueError('hist of shape %s, expected %s' % (tables['hist'].shape, (3, 2, bins)))
    valid = np.zeros(npix, bool)
    if labels is not None:
        lab = np.asarray(labels).ravel().astype(np.int64)
        valid = (lab >= 0) & (lab < C)
    if fixed_row >= 0:
        counted, row = np.ones(npix, bool), np.full(npix, fixed_row, np.int64)
    else:
        counted, row = valid, (np.asarray(win).ravel().astype(np.int64) != lab).astype(np.int64)
    for i, v in enumerate(values):
        np.add.at(tables['hist'][i], (row[counted], bin_index(v, m, o)[counted]), 1)
    if labels is not None:
        tables['counts'] += np.bincount(lab[valid], minlength=C)
        if nll_pixel is not None:
            tables['nll'] += np.bincount(lab[valid], weights=np.asarray(nll_pixel, np.float32).ravel()[valid].astype(np.float64),
                                         minlength=C)
    return tables


class UncertaintyBenchmarks(object):
    """The benchmarks themselves, for any model that can add a batch to the tables: the public methods and what they share.
    A model provides `uncertainty_metrics`, `_uncertainty_state(batch)` and `_uncertainty_accumulate(state, labels, tables,
    temperature, fixed_row)`.  UncertaintyModel (below) provides them from materialised uncertainty maps, BaseModel from the
    confidence of the model's class scores (ops.CONFIDENCE_METRICS).  Config keys: `uncertainty_mantissa_bits` (5),
    `uncertainty_octaves` (24), `reduce_score_over_ranks` (as score())."""

    # ---- hooks -----------------------------------------------------------------------------------------------------------------
    def _uncertainty_state(self, batch):
        """What a batch costs ONCE, whatever is asked of it afterwards (temperature_search reuses it per temperature).  A
        model with experts also takes experts=True: the state must then serve every expert's own tables."""
        raise NotImplementedError

    def _uncertainty_accumulate(self, state, labels, tables, temperature, fixed_row):
        """Adds one batch to `tables` ({'hist' int64 [metrics, 2, bins], 'nll', 'counts'} on the device; with the experts'
        tables asked for also 'experts': the same three with a leading expert axis)."""
        raise NotImplementedError

    def _uncertainty_check(self):
        """Raises NotImplementedError where the model cannot serve the benchmarks; called before anything is allocated."""

    def _uncertainty_experts(self):
        """The names of the experts whose own tables uncertainty_tables(experts=True) returns."""
        raise ValueError('%s has no experts: experts=True is a fusion model\'s' % type(self).__name__)

    # ---- helpers ---------------------------------------------------------------------------------------------------------------
    def _uncertainty_bins(self):
        return _check_bins(self.config.get('uncertainty_mantissa_bits', 5), self.config.get('uncertainty_octaves', 24))

    def _default_temperature(self):
        return self.config.get('temperature_scaling', 1)

    def _temperature(self, temperature=None):
        t = float(self._default_temperature() if temperature is None else temperature)
        if not t > 0:
            raise ValueError('a temperature must be positive')
        return t

    def _metric_index(self, metric):
        if metric not in self.uncertainty_metrics:
            raise UserWarning('ERROR: %s has no uncertainty metric %r (one of %s)' % (
                type(self).__name__, metric, ', '.join(self.uncertainty_metrics)))
        return self.uncertainty_metrics.index(metric)

    def _new_tables(self, experts=False):
        self._uncertainty_check()
        m, o = self._uncertainty_bins()
        tables = ops.uncertainty_tables(self.config['num_classes'], self.device, len(self.uncertainty_metrics), m, o)
        if experts:
            E = len(self._uncertainty_experts())
            tables['experts'] = {k: t.new_zeros((E,) + tuple(t.shape)) for k, t in tables.items()}
        return tables

    def _accumulate(self, data, tables_per_temperature, temperatures, fixed_row=-1):
        from .base_model import iterate_batches
        labels_needed = fixed_row < 0
        experts = 'experts' in tables_per_temperature[0]
        batches = iterate_batches(data, self.config['batchsize'])
        for batch in self._device_batches(batches, labels=labels_needed):
            if labels_needed and 'labels' not in batch:
                raise ValueError('the data carries no labels')
            labels = self._to_device(batch['labels'], torch.int32) if labels_needed else None
            state = self._uncertainty_state(batch, experts=True) if experts else self._uncertainty_state(batch)
            for t, tables in zip(temperatures, tables_per_temperature):
                self._uncertainty_accumulate(state, labels, tables, t, fixed_row)

    def _finish(self, tables):
        from .base_model import reduce_over_ranks
        reduce_over_ranks(self, tables['hist'], tables['nll'], tables['counts'])
        m, o = self._uncertainty_bins()
        out = {'metrics': tuple(self.uncertainty_metrics), 'hist': tables['hist'].cpu().numpy(),
               'nll_sum': tables['nll'].cpu().numpy(), 'counts': tables['counts'].cpu().numpy(), 'edges': bin_edges(m, o)}
        if 'experts' in tables:
            et = tables['experts']
            reduce_over_ranks(self, et['hist'], et['nll'], et['counts'])
            hist, nll, counts = et['hist'].cpu().numpy(), et['nll'].cpu().numpy(), et['counts'].cpu().numpy()
            out['experts'] = {name: dict(out, hist=hist[e], nll_sum=nll[e], counts=counts[e])
                              for e, name in enumerate(self._uncertainty_experts())}
        return out

    @staticmethod
    def _mean_nll(tables):
        with np.errstate(divide='ignore', invalid='ignore'):
            return tables['nll_sum'] / tables['counts']

    # ---- public API ------------------------------------------------------------------------------------------------------------
    def uncertainty_tables(self, data, temperature=None, experts=False, fixed_row=-1):
        """ONE pass over `data` (one set of dropout masks): {'metrics', 'hist' int64 [metrics, 2, bins] (row 1: misclassified),
        'nll_sum' float64 [C], 'counts' int64 [C], 'edges' float64 [bins + 1]} over the pixels with a valid label.
        experts=True (fusion models): also 'experts': {modality: the same tables of that expert's own posterior}.
        fixed_row 0 / 1: every pixel of `data` into that row instead (the out-of-distribution benchmark's halves); labels are
        not read and the NLL sums stay empty."""
        tables = self._new_tables(experts)
        self._accumulate(data, [tables], [self._temperature(temperature)], fixed_row=int(fixed_row))
        return self._finish(tables)

    def misclassification_detection_score(self, data, metric):
        """(fpr, tpr, auroc, thresholds) of `metric` as a detector of the misclassified pixels of `data`."""
        i = self._metric_index(metric)
        t = self.uncertainty_tables(data)
        return roc_from_histogram(t['hist'][i], t['edges'])

    def out_of_distribution_detection_score(self, data, metric, ood_data):
        """(fpr, tpr, auroc, thresholds) of `metric` as a detector of the pixels of `ood_data` among those of `data`: every
        pixel counts, labels are not read."""
        i = self._metric_index(metric)
        tables = self._new_tables()
        t = self._temperature()
        self._accumulate(data, [tables], [t], fixed_row=0)
        self._accumulate(ood_data, [tables], [t], fixed_row=1)
        out = self._finish(tables)
        return roc_from_histogram(out['hist'][i], out['edges'])

    def nll_score(self, data):
        """(nll float64 [C]: mean of -ln(clip(mean[label], 1e-10, 1)) per ground-truth class, NaN for an absent class;
        class_counts int64 [C])"""
        t = self.uncertainty_tables(data)
        return self._mean_nll(t), t['counts']

    def value_distribution(self, data, metric):
        """(counts int64 [bins], edges float64 [bins + 1]) of `metric` over the pixels of `data` with a valid label."""
        i = self._metric_index(metric)
        t = self.uncertainty_tables(data)
        return t['hist'][i].sum(0), t['edges']

    def temperature_search(self, data, temperatures):
        """One entry per temperature: {'temperature', 'nll' (as nll_score), 'class_counts', 'auroc': {metric: AUROC of
        misclassification detection}, 'tables'}.  A batch's state (the Bayesian FCN: its sample scores, i.e. every
        convolution) is obtained ONCE and accumulated once per temperature, so all temperatures see the same masks."""
        temps = [self._temperature(t) for t in temperatures]
        per = [self._new_tables() for _ in temps]
        self._accumulate(data, per, temps)
        out = []
        for t, tables in zip(temps, per):
            res = self._finish(tables)
            out.append({'temperature': t, 'nll': self._mean_nll(res), 'class_counts': res['counts'],
                        'auroc': {m: roc_from_histogram(res['hist'][i], res['edges'])[2]
                                  for i, m in enumerate(res['metrics'])},
                        'tables': res})
        return out


class UncertaintyModel(UncertaintyBenchmarks):
    """Mixin for models with per-pixel uncertainty maps.  A model provides `_uncertainty_state(batch)` -- by default its maps,
    from `_uncertainty_maps(batch)`: {'label' int64 [N,H,W], 'mean' float32 [N,H,W,C], and one float32 [N,H,W] map per metric
    in `uncertainty_metrics`} -- and may override `_uncertainty_accumulate` (the default bins the maps with
    xv_uncertainty_stats, one launch per metric).  Config keys: `uncertainty_mantissa_bits` (5), `uncertainty_octaves` (24),
    `temperature_scaling` (1), `reduce_score_over_ranks` (as score())."""

    uncertainty_metrics = METRICS
    # (a model is this mixin in front of a BaseModel, which serves the benchmarks from its class scores: what the maps decide
    # is restated here, so that the mixin's answer is found first)
    _default_temperature = UncertaintyBenchmarks._default_temperature
    _uncertainty_check = UncertaintyBenchmarks._uncertainty_check
    _uncertainty_experts = UncertaintyBenchmarks._uncertainty_experts

    def _uncertainty_maps(self, batch):
        raise NotImplementedError

    def _uncertainty_state(self, batch):
        """What a batch costs ONCE, whatever is asked of it afterwards (temperature_search reuses it per temperature)."""
        return self._uncertainty_maps(batch)

    def _uncertainty_accumulate(self, state, labels, tables, temperature, fixed_row):
        """Adds one batch to `tables` ({'hist' int64 [metrics, 2, bins], 'nll', 'counts'} on the device)."""
        if float(temperature) != 1.0:
            raise NotImplementedError('%s: the maps of this model have no temperature (temperature_scaling must be 1)'
                                      % type(self).__name__)
        m, o = self._uncertainty_bins()
        for i, metric in enumerate(self.uncertainty_metrics):
            ops.uncertainty_stats(state[metric], state['label'], labels, self.config['num_classes'],
                                  mean_prob=state['mean'] if i == 0 and labels is not None else None, fixed_row=fixed_row,
                                  mantissa_bits=m, octaves=o,
                                  tables={'hist': tables['hist'][i], 'nll': tables['nll'], 'counts': tables['counts']})
