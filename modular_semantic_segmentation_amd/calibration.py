"""Calibration scoring on the host (numpy only, no GPU): the float64 reference of the reliability table the kernels of
csrc/calibration.hip count, and the measures read off such a table -- ECE, MCE, over-confidence, NLL and the diagram.

The table.  A pixel has class scores s[k], k < C, in the log domain (a fusion's class scores, an expert's logits, or
ln(1e-20 + p) of a probability map) and a winner `win`, the first maximum.  Per temperature T > 0
    z = sum_k exp((s[k] - s[win]) / T),  conf = 1 / z,  q = int(conf 2^24),  bin = min(q >> (24 - bin_bits), NB - 1)
with NB = 1 << bin_bits, and over the pixels with 0 <= label < C
    table[t][bin] += (1, win == label, q)                            int64 [T, NB, 3]
    nll[t]        += min(ln z - (s[label] - s[win]) / T, -ln 1e-10)  float64 [T]
The three columns are integers, so tables of groups, ranks and batches add exactly; the mean confidence of a bin is its q sum
over its count, in steps of 2^-24."""
import numpy as np

Q_ONE = 1 << 24                          # the fixed-point confidence 1
NLL_CLIP = -np.log(1e-10)                # the clip of the NLL term, as the uncertainty benchmarks have it


def table_reference(values, labels, temperatures, bin_bits, kind=0, groups=None, num_groups=1):
    """The table in float64: values [n, ..., C] (kind 0: scores in the log domain; kind 1: probabilities, whose winner is taken
    first and which then become ln(1e-20 + p)), labels int [n, ...], temperatures a sequence of T > 0, bin_bits in 4..10.
    groups: one id per image; an id outside [0, num_groups) counts nothing.  Returns (table int64 [T, NB, 3], nll float64 [T],
    conf float64 [T, n, ...]) -- table and nll with a leading [num_groups] axis when groups are given; conf is every pixel's
    confidence at every temperature, void pixels included."""
    v = np.asarray(values, np.float64)
    lab = np.asarray(labels).astype(np.int64)
    temps = [float(t) for t in np.atleast_1d(np.asarray(temperatures, np.float64))]
    if not 4 <= int(bin_bits) <= 10:
        raise ValueError('bin_bits must lie in 4..10, got %r' % (bin_bits,))
    if not temps or not all(np.isfinite(t) and t > 0 for t in temps):
        raise ValueError('temperatures must be finite and positive, got %r' % (temperatures,))
    if kind not in (0, 1):
        raise ValueError('kind must be 0 or 1, got %r' % (kind,))
    C, NB = v.shape[-1], 1 << int(bin_bits)
    if v.shape[:-1] != lab.shape or lab.ndim < 1:
        raise ValueError('values of shape %s, labels of shape %s' % (v.shape, lab.shape))
    win = np.argmax(v, -1)                                  # (numpy's argmax is the first maximum)
    s = np.log(np.float64(np.float32(1e-20)) + v) if kind == 1 else v
    s_win = np.take_along_axis(s, win[..., None], -1)
    valid = (lab >= 0) & (lab < C)
    s_lab = np.take_along_axis(s, np.where(valid, lab, 0)[..., None], -1)[..., 0]
    n = lab.shape[0]
    NG = int(num_groups)
    ids = np.zeros(n, np.int64) if groups is None else np.asarray(groups).astype(np.int64)
    if ids.shape != (n,):
        raise ValueError('groups must hold one id per image')
    pix_group = np.broadcast_to(ids.reshape((n,) + (1,) * (lab.ndim - 1)), lab.shape)
    counted = valid & (pix_group >= 0) & (pix_group < NG)
    table = np.zeros((NG, len(temps), NB, 3), np.int64)
    nll = np.zeros((NG, len(temps)), np.float64)
    conf = np.zeros((len(temps),) + lab.shape, np.float64)
    for t, T in enumerate(temps):
        z = np.exp((s - s_win) / T).sum(-1)
        conf[t] = 1.0 / z
        q = np.floor(conf[t] * Q_ONE).astype(np.int64)
        b = np.minimum(q >> (24 - int(bin_bits)), NB - 1)
        term = np.minimum(np.log(z) - (s_lab - s_win[..., 0]) / T, NLL_CLIP)
        g, bb = pix_group[counted], b[counted]
        np.add.at(table[:, t, :, 0], (g, bb), 1)
        np.add.at(table[:, t, :, 1], (g, bb), (win == lab)[counted].astype(np.int64))
        np.add.at(table[:, t, :, 2], (g, bb), q[counted])
        np.add.at(nll[:, t], g, term[counted])
    if groups is None:
        return table[0], nll[0], conf
    return table, nll, conf


def regroup(table, num_bins):
    """A table [..., NB, 3] on `num_bins` coarser bins: fine bin b goes to floor(b num_bins / NB).  Exact where num_bins
    divides NB (every coarse edge is a fine edge); otherwise a coarse edge j / num_bins lies inside one fine bin, whose pixels
    all go to the side of its lower edge -- the grouping is right to within one fine bin (2^-bin_bits of confidence) at each
    edge."""
    t = np.asarray(table)
    NB, num_bins = t.shape[-2], int(num_bins)
    if t.shape[-1] != 3 or not 1 <= num_bins <= NB:
        raise ValueError('table of shape %s for %d bins' % (t.shape, num_bins))
    to = (np.arange(NB, dtype=np.int64) * num_bins) // NB
    out = np.zeros(t.shape[:-2] + (num_bins, 3), t.dtype)
    np.add.at(out, (Ellipsis, to, slice(None)), t)
    return out


def calibration_measures(table, nll, num_bins=15):
    """Measures of ONE reliability table (int [NB, 3], one temperature) and its NLL sum:
      ECE              sum_b n_b / N |acc_b - conf_b| over the `num_bins` regrouped bins, conf_b the bin's mean confidence
                       (its q sum / 2^24 / n_b), acc_b its share of correct pixels
      MCE              the largest |acc_b - conf_b| of a non-empty bin
      accuracy         correct / N
      mean_confidence  q sum / 2^24 / N
      overconfidence   mean_confidence - accuracy
      NLL              nll / N
      pixels           N
      diagram          {edges [num_bins + 1] (the fine-bin edges regroup cuts at), count, accuracy, confidence [num_bins]; an
                       empty bin gives NaN}
    A table without pixels gives NaN."""
    t = np.asarray(table)
    if t.ndim != 2 or t.shape[1] != 3:
        raise ValueError('calibration table of shape %s, expected [NB, 3]' % (t.shape,))
    NB = t.shape[0]
    g = regroup(t, num_bins).astype(np.float64)
    count, right, conf = g[:, 0], g[:, 1], g[:, 2] / Q_ONE
    N = count.sum()
    with np.errstate(divide='ignore', invalid='ignore'):
        acc_b, conf_b = right / count, conf / count
        gap = np.where(count > 0, np.abs(acc_b - conf_b), 0.0)
        measures = {'ECE': float((count * gap).sum() / N), 'MCE': float(gap.max()) if N > 0 else float('nan'),
                    'accuracy': float(right.sum() / N), 'mean_confidence': float(conf.sum() / N),
                    'NLL': float(np.float64(nll) / N), 'pixels': int(N)}
    measures['overconfidence'] = measures['mean_confidence'] - measures['accuracy']
    edges = -((-np.arange(num_bins + 1, dtype=np.int64) * NB) // int(num_bins)) / float(NB)       # ceil(j NB / num_bins) / NB
    measures['diagram'] = {'edges': edges, 'count': g[:, 0].astype(np.int64), 'accuracy': acc_b, 'confidence': conf_b}
    return measures


def best_temperature(temperatures, measures):
    """The temperature of least NLL among `measures` (one calibration_measures result per temperature; the first on ties)."""
    return float(temperatures[int(np.argmin([m['NLL'] for m in measures]))])


def confidence_reference(values, temperature, kind=0):
    """The maps of csrc/confidence.hip in float64: values [..., C] (kind 0: scores in the log domain; kind 1: probabilities,
    whose winner is taken first and which then become ln(1e-20 + p)) at ONE temperature T > 0.  Returns (label int64 [...], the
    first maximum; confidence = 1 / z with z = sum_k e_k, e_k = exp(d_k), d_k = (s[k] - s[label]) / T; entropy = max(0, ln z -
    (sum_k e_k d_k) / z) in nats, a term with e_k = 0 adding nothing; margin = confidence - max_{k != label} e_k / z)."""
    v = np.asarray(values, np.float64)
    T = float(temperature)
    if not (np.isfinite(T) and T > 0):
        raise ValueError('the temperature must be finite and positive, got %r' % (temperature,))
    if kind not in (0, 1):
        raise ValueError('kind must be 0 or 1, got %r' % (kind,))
    if v.ndim < 1 or v.shape[-1] < 2:
        raise ValueError('values of shape %s, expected [..., C] with C >= 2' % (v.shape,))
    win = np.argmax(v, -1)                                  # (numpy's argmax is the first maximum)
    s = np.log(np.float64(np.float32(1e-20)) + v) if kind == 1 else v
    d = (s - np.take_along_axis(s, win[..., None], -1)) / T
    e = np.exp(d)
    z = e.sum(-1)
    with np.errstate(invalid='ignore'):
        ed = np.where(e > 0, e * d, 0.0).sum(-1)
    others = np.where(np.arange(v.shape[-1]) == win[..., None], -np.inf, e)
    conf = 1.0 / z
    return win.astype(np.int64), conf, np.maximum(np.log(z) - ed / z, 0.0), conf - others.max(-1) / z


def risk_coverage(table):
    """Selective prediction read off ONE reliability table (int [NB, 3]): keeping only the pixels whose fixed-point confidence
    q is at least j 2^24 / NB -- what a confidence map's threshold j / NB keeps, the lower edge of bin j -- for every j < NB:
      thresholds [NB]  j / NB
      coverage   [NB]  the share of the counted pixels that is kept (the bins j and above)
      risk       [NB]  1 - accuracy among the kept ones; NaN where none is kept
      area             the area under risk over coverage by the trapezoid rule, the curve continued flat from its smallest
                       coverage down to 0 (a constant risk gives that risk); NaN for a table without pixels
    The counts are integers, so coverage and risk are exact ratios of them."""
    t = np.asarray(table)
    if t.ndim != 2 or t.shape[1] != 3:
        raise ValueError('calibration table of shape %s, expected [NB, 3]' % (t.shape,))
    NB = t.shape[0]
    kept = np.cumsum(t[::-1, 0].astype(np.int64))[::-1]
    right = np.cumsum(t[::-1, 1].astype(np.int64))[::-1]
    N = int(kept[0])
    with np.errstate(divide='ignore', invalid='ignore'):
        coverage = kept / np.float64(N) if N > 0 else np.full(NB, np.nan)
        risk = np.where(kept > 0, 1.0 - right / kept.astype(np.float64), np.nan)
    area = float('nan')
    if N > 0:
        keep = kept > 0
        c, r = coverage[keep][::-1], risk[keep][::-1]       # ascending coverage
        area = float(c[0] * r[0] + ((c[1:] - c[:-1]) * (r[1:] + r[:-1]) / 2).sum())
    return {'thresholds': np.arange(NB) / float(NB), 'coverage': coverage, 'risk': risk, 'area': area}
