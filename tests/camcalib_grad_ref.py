"""Float64 NumPy yardstick of CamCalib's differentiable tail: CameraRegressorLoss (camcalib/loss.py:24-125) and the three FC heads
(camcalib/model.py:59-70), each with a HAND-WRITTEN backward, and the seeded cases the host and GPU tests share.

The loss, per row x (nbins logits) of head k with p = softmax(x), E = sum_i i p_i, s = 2 E / (n - 1) - 1:
    'ce' / 'kl'             term = log sum exp(x - max) - (x_t - max),   d term / d x_i = p_i - [i == t]
    'softargmax_l2'         term = (t - s)^2,                            d term / d x_i = -2 (t - s) (2 / (n - 1)) p_i (i - E)
    'softargmax_biased_l2'  vfov only: term = l2 / (l2 + 1) wherever s > t is false, slope -2 (t - s) / (l2 + 1)^2
head loss = weight x batch mean of the term, loss = the sum of the three.  i - E is formed relative to the arg-max bin m,
i - E = (i - m) - sum_i p_i (i - m): the same number, but on a nearly one-hot row E rounds to the integer m even in float64 (a
neighbour's share of 1e-34 is below the spacing of doubles at m) and the plain difference would return 0 for the bin m.
"""
import numpy as np

from tests import head_ref

LOSS_TYPES = ('ce', 'kl', 'softargmax_l2', 'softargmax_biased_l2')
WEIGHTS = (1.5, 0.5, 2.0)                      # unequal: a swapped head shows
LOSS_KEYS = ('loss', 'vfov_loss', 'pitch_loss', 'roll_loss')
# the cases of tests/golden/camcalib_loss_grad.npz: (B, nbins, the logits' scale).  3 N(0, 1) over 256 bins is what a trained head
# emits; over 65 bins the same scale leaves rows that are nearly one-hot, where the fp32 autograd the fixture holds loses digits
# itself (7e-6 of the largest gradient) - that regime is `saturated_case`'s, with a bound of its own - so the small case is N(0, 1)
FIXTURE_CASES = {'b5n256': (5, 256, 3.0), 'b3n65': (3, 65, 1.0), 'b4n2': (4, 2, 3.0)}
SATURATED_ROWS = (0, 1, 2, 3, head_ref.BIG_ROW)   # of head_ref.decode_rows: one-hot first / middle / last, all equal, spans +-1e4


def loss_case(B, nbins, loss_type, scale=3.0):
    """logits (3, B, nbins) float32 = scale N(0, 1); targets (3, B): int64 bins for 'ce' / 'kl', float32 in [-1, 1] otherwise."""
    rng = np.random.default_rng([1, B, nbins])
    logits = (scale * rng.standard_normal((3, B, nbins))).astype(np.float32)
    bins = rng.integers(0, nbins, (3, B)).astype(np.int64)
    soft = rng.uniform(-1, 1, (3, B)).astype(np.float32)
    return logits, (bins if loss_type in ('ce', 'kl') else soft)


def saturated_case(nbins, loss_type):
    """The five saturated rows of ``head_ref.decode_rows`` as one batch: logits (3, 5, nbins); targets on and off the hot bins."""
    x = head_ref.decode_rows(nbins)[0][:, list(SATURATED_ROWS)].copy()
    hot = head_ref.one_hot_bins(nbins)
    bins = np.array([hot[0], nbins - 1, hot[2], nbins // 3, nbins - 1], np.int64)
    soft = np.array([-1.0, 0.3, 0.9, -0.2, 0.5], np.float32)
    t = bins if loss_type in ('ce', 'kl') else soft
    return x, np.stack([t, t[::-1].copy(), np.roll(t, 2)])


def camcalib_loss(logits, targets, loss_type, weights=WEIGHTS, g_means=(1.0, 0.0, 0.0, 0.0)):
    """-> (terms (3, B), means (4,), grads (3, B, nbins)), float64; grads = the gradient of sum_j g_means[j] means[j]."""
    x = np.asarray(logits, np.float64)
    _, B, n = x.shape
    gm = np.asarray(g_means, np.float64)
    terms, grads = np.zeros((3, B)), np.zeros((3, B, n))
    idx = np.arange(n, dtype=np.float64)
    for k in range(3):
        c = weights[k] * (gm[0] + gm[1 + k]) / B
        for b in range(B):
            r = x[k, b]
            m = int(np.argmax(r))
            e = np.exp(r - r[m])
            se = e.sum()
            p = e / se
            if loss_type in ('ce', 'kl'):
                t = int(min(max(int(targets[k][b]), 0), n - 1))
                terms[k, b] = np.log(se) - (r[t] - r[m])
                g = p.copy()
                g[t] = -e[idx != t].sum() / se           # p_t - 1 = -(the other bins' share), without the cancellation
                grads[k, b] = c * g
            else:
                t = float(np.float32(targets[k][b]))
                rel = idx - m
                Erel = (p * rel).sum()
                s = 2.0 * (m + Erel) / (n - 1) - 1.0
                d = t - s
                l2 = d * d
                slope = -2.0 * d
                if loss_type == 'softargmax_biased_l2' and k == 0 and not s > t:
                    terms[k, b] = l2 / (l2 + 1.0)
                    slope /= (l2 + 1.0) ** 2
                else:
                    terms[k, b] = l2
                grads[k, b] = c * slope * (2.0 / (n - 1)) * p * (rel - Erel)
    head = np.array([weights[k] * terms[k].mean() for k in range(3)])
    means = np.array([head.sum(), *head])
    return terms, means, grads


def row_err(got, want):
    """max over the rows of max|got - want| / max|want| of the row; a row whose yardstick is all zero must be all zero."""
    got, want = np.asarray(got, np.float64).reshape(-1, np.shape(want)[-1]), np.asarray(want, np.float64).reshape(-1, np.shape(want)[-1])
    worst = 0.0
    for g, w in zip(got, want):
        top = np.abs(w).max()
        if top == 0:
            assert not g.any(), 'a row whose gradient is exactly zero came back non-zero'
            continue
        worst = max(worst, float(np.abs(g - w).max() / top))
    return worst


def err(got, want):
    """max|got - want| / max|want|: the largest deviation in units of the tensor's largest magnitude."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


# ---- the three FC chains ---------------------------------------------------------------------------------------------------------
HEADS = ('fc_vfov', 'fc_pitch', 'fc_roll')
# (B, F, L, Hc, nbins): tails in every dimension, one shape per path and one at the real size (Hc is not read with L = 1)
HEAD_SHAPES = ((1, 1, 1, 1, 2), (3, 40, 2, 33, 65), (33, 65, 3, 31, 257), (65, 2048, 1, 1, 256), (2, 2048, 3, 1024, 256))
TRAIN_SHAPE = (3, 40, 2, 33, 65)


def param_names(L):
    return tuple(f'{h}.{kind}' if L == 1 else f'{h}.{l}.{kind}' for h in HEADS for l in range(L) for kind in ('weight', 'bias'))


def head_case(B, F, L, Hc, nbins):
    """params {state_dict name: float32 array} (uniform +-1 / sqrt(fan_in), nn.Linear's range), xf (B, F), g_logits (3, B, nbins)."""
    rng = np.random.default_rng([2, B, F, L, Hc, nbins])
    params = {}
    for h in HEADS:
        for l in range(L):
            nin, nout = (F if l == 0 else Hc), (nbins if l == L - 1 else Hc)
            stem = h if L == 1 else f'{h}.{l}'
            params[f'{stem}.weight'] = (rng.uniform(-1, 1, (nout, nin)) / np.sqrt(nin)).astype(np.float32)
            params[f'{stem}.bias'] = (rng.uniform(-1, 1, nout) / np.sqrt(nin)).astype(np.float32)
    xf = rng.standard_normal((B, F)).astype(np.float32)
    g_logits = rng.standard_normal((3, B, nbins)).astype(np.float32)
    return params, xf, g_logits


def chain_forward(params, xf, L):
    """-> (logits (3, B, nbins), acts[k][l] = the input of layer l of head k), float64."""
    names = param_names(L)
    logits, acts = [], []
    for k in range(3):
        a, mine = np.asarray(xf, np.float64), []
        for l in range(L):
            mine.append(a)
            w, b = (np.asarray(params[names[(k * L + l) * 2 + i]], np.float64) for i in (0, 1))
            a = a @ w.T + b
        logits.append(a)
        acts.append(mine)
    return np.stack(logits), acts


def chain_backward(params, xf, L, g_logits):
    """-> (g_xf (B, F), {name: gradient}), float64: G_L = g_logits, G_{l-1} = G_l W_l, dW_l = G_l^T A_{l-1}, db_l = column sums."""
    names = param_names(L)
    _, acts = chain_forward(params, xf, L)
    grads, g_xf = {}, 0.0
    for k in range(3):
        G = np.asarray(g_logits[k], np.float64)
        for l in range(L - 1, -1, -1):
            wn, bn = names[(k * L + l) * 2], names[(k * L + l) * 2 + 1]
            grads[wn] = G.T @ acts[k][l]
            grads[bn] = G.sum(0)
            G = G @ np.asarray(params[wn], np.float64)
        g_xf = g_xf + G
    return g_xf, grads


# ---- features -> heads -> loss, and plain gradient descent on it ------------------------------------------------------------------
def tail_grads(params, xf, L, targets, loss_type, weights=WEIGHTS):
    """-> (means (4,), g_xf, {name: gradient}) of ``loss`` through the three chains, float64."""
    logits, _ = chain_forward(params, xf, L)
    _, means, g_logits = camcalib_loss(logits, targets, loss_type, weights)
    g_xf, grads = chain_backward(params, xf, L, g_logits)
    return means, g_xf, grads


SGD_STEPS = 6
# Chosen on the float64 chain below: at 0.01 every one of the six steps lowers the loss for all four loss types (by about 3 % a
# step for 'ce' / 'kl', 0.3 % for the soft-argmax losses), and ten times the rate still descends - the margin an fp32 run needs.
# tests/test_camcalib_grad_host.py checks both.
SGD_RATE = 0.01


def sgd_losses(loss_type, steps=SGD_STEPS, rate=SGD_RATE):
    """The loss before each of ``steps`` steps of plain gradient descent on the parameters, and after the last: steps + 1 values."""
    B, F, L, Hc, nbins = TRAIN_SHAPE
    params, xf, _ = head_case(*TRAIN_SHAPE)
    params = {k: np.asarray(v, np.float64) for k, v in params.items()}
    _, targets = loss_case(B, nbins, loss_type)
    out = []
    for _ in range(steps + 1):
        means, _, grads = tail_grads(params, xf, L, targets, loss_type)
        out.append(float(means[0]))
        params = {k: v - rate * grads[k] for k, v in params.items()}
    return out
