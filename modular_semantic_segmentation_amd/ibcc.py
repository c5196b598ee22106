"""Variational IBCC (independent Bayesian classifier combination; Kim & Ghahramani 2012, Simpson et al. 2013) on the host.

The reference's experiments/ibcc_fusion.py only dumps every expert's label maps for an external IBCC.  IBCC's likelihood sees
a pixel only through the tuple of its experts' labels, t = ((l_0 C + l_1) C + l_2) ... (expert 0 most significant, the
row-major index of bayes_decision_matrix's [C]*E array), so a whole dataset is ONE histogram over the T = C^E tuples
(ops.fused_head_multi_tuple_hist counts it on the device, without ground truth) and the variational updates run on that
histogram here, in float64 numpy, in microseconds per iteration -- the split of dirichlet_fit.py: the counting on the device,
a tiny solve on the host.  The fitted model is again a function of the tuple: a lookup table.

Model: true class j ~ Cat(kappa), kappa ~ Dir(nu0); expert e answers l with probability pi^e[j][l], pi^e[j] ~ Dir(alpha0^e[j]).
With psi the digamma function the updates are

    E[ln kappa_j]    = psi(nu_j) - psi(sum_j nu_j)
    E[ln pi^e_jl]    = psi(alpha^e_jl) - psi(sum_l alpha^e_jl)
    ln rho_tj        = E[ln kappa_j] + sum_e E[ln pi^e_{j, l_e(t)}]          q(j|t) = softmax_j ln rho_tj
    nu_j             = nu0_j + sum_t hist[t] q(j|t)
    alpha^e_jl       = alpha0^e_jl + sum_{t: l_e(t) = l} hist[t] q(j|t)
"""
from collections import namedtuple

import numpy as np
from scipy.special import gammaln, psi

IbccResult = namedtuple('IbccResult', 'alpha nu posterior lut iterations lower_bounds converged')
IbccResult.__doc__ = """alpha float64 [E, C, C] (true class x answer) and nu float64 [C]: the posterior Dirichlet parameters;
posterior float64 [T, C]: q(j|t) under them; lut uint8 [T]: its first-maximum argmax; iterations: how many were run;
lower_bounds float64 [iterations]: the variational lower bound after every iteration; converged: max |dq| < tol was reached."""


def tuple_index(labels, num_classes):
    """t = ((l_0 C + l_1) C + l_2) ... of E label arrays (expert 0 most significant), as int64: the row-major index of a
    [C]*E decision array such as bayes_decision_matrix's."""
    labels = [np.asarray(l, np.int64) for l in labels]
    t = np.zeros_like(labels[0])
    for l in labels:
        t = t * int(num_classes) + l
    return t


def tuple_labels(num_classes, num_experts):
    """int64 [E, T]: l_e(t), the label of expert e in tuple t."""
    C, E = int(num_classes), int(num_experts)
    return np.stack(np.unravel_index(np.arange(C ** E), (C,) * E)).astype(np.int64)


def _expected_logs(alpha, nu):
    return psi(alpha) - psi(alpha.sum(-1, keepdims=True)), psi(nu) - psi(nu.sum())


def _log_rho(elnpi, elnkappa, digits):
    """float64 [T, C]: ln rho_tj, the experts added in ascending order."""
    lnrho = np.broadcast_to(elnkappa, (digits.shape[1], len(elnkappa))).copy()
    for e in range(len(digits)):
        lnrho += elnpi[e][:, digits[e]].T
    return lnrho


def _softmax_rows(lnrho):
    """(q, ln q) of the rows."""
    shifted = lnrho - lnrho.max(-1, keepdims=True)
    lnq = shifted - np.log(np.exp(shifted).sum(-1, keepdims=True))
    return np.exp(lnq), lnq


def _dirichlet_kl(a, b):
    """sum over the leading axes of KL(Dir(a) || Dir(b)), the last axis being the Dirichlet's."""
    sa = a.sum(-1)
    kl = gammaln(sa) - gammaln(a).sum(-1) - gammaln(b.sum(-1)) + gammaln(b).sum(-1) + \
        ((a - b) * (psi(a) - psi(sa)[..., None])).sum(-1)
    return float(np.sum(kl))


def _lower_bound(hist, q, lnq, alpha, nu, alpha0, nu0, digits):
    """E_q[ln p(data, classes, pi, kappa)] - E_q[ln q] for the responsibilities q and the Dirichlets (alpha, nu)."""
    lnrho = _log_rho(*_expected_logs(alpha, nu), digits)
    data = float(np.sum(hist[:, None] * q * (lnrho - lnq)))
    return data - _dirichlet_kl(nu, nu0) - _dirichlet_kl(alpha, alpha0)


def vb_ibcc(hist, alpha0, nu0, max_iter=200, tol=1e-6):
    """Variational IBCC on the tuple histogram.  hist [T] (T = C^E, any integer or float dtype; the tuple index above), alpha0
    [E, C, C] (true class x answer) and nu0 [C] the Dirichlet priors.  Every iteration takes q from the current Dirichlets and
    then the Dirichlets from q, starting at the priors, until max |q - q of the iteration before| < tol (over the tuples that
    occur: the others carry no weight) or max_iter iterations were run (max_iter = 0: none).  Returns an IbccResult whose
    posterior is q under the final Dirichlets.  hist == 0: there is nothing to iterate on -- the Dirichlets are the priors,
    the posterior their own decision, no iteration is run and the result counts as converged."""
    alpha0, nu0 = np.asarray(alpha0, np.float64), np.asarray(nu0, np.float64)
    if alpha0.ndim != 3 or alpha0.shape[1] != alpha0.shape[2] or nu0.shape != alpha0.shape[1:2]:
        raise ValueError('alpha0 of shape %s and nu0 of shape %s, expected [E, C, C] and [C]' % (alpha0.shape, nu0.shape))
    if not (np.all(alpha0 > 0) and np.all(nu0 > 0)):
        raise ValueError('Dirichlet priors must be positive')
    E, C = alpha0.shape[:2]
    hist = np.asarray(hist, np.float64).reshape(-1)
    if hist.shape != (C ** E,) or np.any(hist < 0):
        raise ValueError('hist of %d bins, expected C^E = %d non-negative counts' % (hist.size, C ** E))
    digits = tuple_labels(C, E)
    # a tuple nobody answered enters no sum: the iterations run on the tuples that occur, the table over all T of them is taken
    # once at the end
    seen = np.flatnonzero(hist)
    counts, seen_digits = hist[seen], digits[:, seen]
    answered = [np.eye(C)[seen_digits[e]] for e in range(E)]      # [seen, l]: one-hot answers of expert e
    alpha, nu = alpha0.copy(), nu0.copy()
    bounds, q_old, converged, iterations = [], None, len(seen) == 0, 0
    for iterations in range(1, int(max_iter) + 1 if len(seen) else 0):
        q, lnq = _softmax_rows(_log_rho(*_expected_logs(alpha, nu), seen_digits))
        w = counts[:, None] * q                                   # [seen, j]
        nu = nu0 + w.sum(0)
        alpha = np.stack([alpha0[e] + (answered[e].T @ w).T for e in range(E)])
        bounds.append(_lower_bound(counts, q, lnq, alpha, nu, alpha0, nu0, seen_digits))
        if q_old is not None and np.max(np.abs(q - q_old)) < tol:
            converged = True
            break
        q_old = q
    posterior, _ = _softmax_rows(_log_rho(*_expected_logs(alpha, nu), digits))
    return IbccResult(alpha, nu, posterior, np.argmax(posterior, -1).astype(np.uint8), iterations,
                      np.asarray(bounds, np.float64), converged)


def ibcc_priors(confusion_matrices, prior_strength=None):
    """(alpha0 float64 [E, C, C], nu0 float64 [C]) from E confusion matrices [C, C] with rows = ground truth, columns = the
    expert's answer (a BayesFusion holds their transposes).  prior_strength None: the measured pixels count as observations,
    alpha0^e = 1 + cm_e and nu0 = 1 + the class counts of the LAST expert's matrix (the matrix bayes_mix._prior takes the data
    prior from).  A number s: every true-class row is rescaled to s pseudo-observations, 1 + s cm[j, :] / sum cm[j, :] (an
    empty row stays 1), and nu0 to s C in total."""
    cms = [np.asarray(m, np.float64) for m in confusion_matrices]
    if not cms or any(m.ndim != 2 or m.shape != cms[0].shape or m.shape[0] != m.shape[1] for m in cms):
        raise ValueError('confusion matrices must be E square matrices of one size')
    if any(np.any(m < 0) for m in cms):
        raise ValueError('confusion matrices hold counts: no negative entries')
    C = cms[0].shape[0]
    counts = cms[-1].sum(1)
    if prior_strength is None:
        return 1.0 + np.stack(cms), 1.0 + counts
    s = float(prior_strength)
    if s < 0:
        raise ValueError('prior_strength must not be negative')
    rows = np.stack(cms).sum(-1, keepdims=True)
    with np.errstate(divide='ignore', invalid='ignore'):
        alpha0 = 1.0 + s * np.where(rows > 0, np.stack(cms) / rows, 0.0)
        nu0 = 1.0 + (s * C * counts / counts.sum() if counts.sum() > 0 else np.zeros(C))
    return alpha0, nu0
