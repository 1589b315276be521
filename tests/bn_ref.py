"""The float64 reference of BatchNorm in training mode (``specmi_batchnorm_train_forward`` / ``specmi_batchnorm_backward``,
spec_amd/csrc/bn_train.hip) and of a stage of bottlenecks on batch statistics (``spec_amd.differentiable.ResNetStage(bn='batch')``),
written directly from the formulas - no ``F.batch_norm``, no autograd - in torch CPU tensors.

z (M, C):  mean = sum_m z / M,  var = sum_m (z - mean)^2 / M (biased),  invstd = 1 / sqrt(var + eps),
pre = (z - mean) invstd gamma + beta [+ residual],  y = relu ? max(pre, 0) : pre,
running_mean = (1 - f) running_mean + f mean,  running_var = (1 - f) running_var + f var M / (M - 1).
Backward from g_y:  g = relu ? (pre > 0 ? g_y : 0) : g_y  (the mask from the reference's OWN pre-activation; an exact zero passes
no gradient),  g_res = g,  g_beta = sum_m g,  g_gamma = sum_m g xhat,  xhat = (z - mean) invstd,
g_z = gamma invstd (g - g_beta / M - xhat g_gamma / M).

Every input of a case is rounded to fp32 first and then held in float64, so the device reads exactly the reference's numbers (it
matters for the offset case: z ~ N(100, 1) has 7.6e-6 between neighbouring floats).  Mask condition, as in tests/conv_grad_ref.py:
a case with relu is usable only if no float64 pre-activation lies within BAND * max|pre| of zero; the generators walk seeds upward
until the band is empty.
"""
import torch

from tests import conv_grad_ref as R

BAND = R.BAND
EPS = 1e-5
err = R.err


def forward(z, gamma, beta, eps=EPS, residual=None, relu=False, running_mean=None, running_var=None, f=0.1):
    """-> dict(y, pre, mean, var, invstd, running_mean, running_var); the running statistics are returned, not written."""
    M = z.shape[0]
    mean = z.sum(0) / M
    d = z - mean
    var = (d * d).sum(0) / M
    invstd = 1.0 / torch.sqrt(var + eps)
    pre = d * invstd * gamma + beta
    if residual is not None:
        pre = pre + residual
    out = dict(y=pre.clamp_min(0) if relu else pre, pre=pre, mean=mean, var=var, invstd=invstd, running_mean=None, running_var=None)
    if running_mean is not None:
        out['running_mean'] = (1 - f) * running_mean + f * mean
        out['running_var'] = (1 - f) * running_var + f * var * M / (M - 1)
    return out


def backward(z, gamma, mean, invstd, pre, g_y, relu=False):
    """-> (g_z, g_gamma, g_beta, g_res); pre = the pre-activation ``forward`` returned (read only with relu)."""
    M = z.shape[0]
    g = torch.where(pre > 0, g_y, torch.zeros_like(g_y)) if relu else g_y
    xhat = (z - mean) * invstd
    g_beta = g.sum(0)
    g_gamma = (g * xhat).sum(0)
    return gamma * invstd * (g - g_beta / M - xhat * g_gamma / M), g_gamma, g_beta, g


def _f32(t):
    return t.float().double()


def _tensors(M, C, seed, offset):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    t = dict(z=rn(M, C) + (100.0 if offset else 0.0), gamma=0.5 + torch.rand(C, generator=g, dtype=torch.float64), beta=0.3 * rn(C),
             res=rn(M, C), g_y=rn(M, C), running_mean=rn(C), running_var=0.5 + torch.rand(C, generator=g, dtype=torch.float64))
    return {k: _f32(v) for k, v in t.items()}


def case(M, C, base_seed=0, offset=False):
    """The tensors of one (M, C) case (float64 holding fp32 values) with ``seed`` and ``seed_steps``: the mask condition holds with
    and without the residual.  ``offset``: z ~ N(100, 1), the case an uncentred variance fails."""
    for step in range(256):           # (the largest test shape, (129, 130) twice, keeps its band empty at one seed in about 40)
        t = _tensors(M, C, base_seed + 1000 * step + 7 * M + C, offset)
        pres = [forward(t['z'], t['gamma'], t['beta'], EPS, res)['pre'] for res in (None, t['res'])]
        if R.band_empty(pres):
            t.update(M=M, C=C, seed_steps=step)
            return t
    raise RuntimeError(f'no seed with an empty band for {(M, C)}')


def uncentred_y_fp32(z, gamma, beta, eps=EPS):
    """y with var = E[z^2] - E[z]^2 evaluated in fp32: what the kernels must NOT do (the offset case exists to catch it)."""
    z, gamma, beta = z.float(), gamma.float(), beta.float()
    mean = z.mean(0)
    var = (z * z).mean(0) - mean * mean
    return (z - mean) / torch.sqrt(var + eps) * gamma + beta


# ---- a stage of bottlenecks on batch statistics -------------------------------------------------------------------------------
def _conv_bn(x, c, stride, pad, stat, eps, res=None, relu=True):
    """conv as a plain product, then BatchNorm on the statistics of the batch -> (rec, out); x / out NHWC."""
    ones, zeros = torch.ones_like(c['scale']), torch.zeros_like(c['shift'])
    z = R.layer_forward(x, c['w'], ones, zeros, stride, pad, None, False)[0]
    C = z.shape[-1]
    f = forward(z.reshape(-1, C), c['scale'], c['shift'], eps, None if res is None else res.reshape(-1, C), relu, stat['running_mean'],
                stat['running_var'], stat['f'])
    return dict(x=x, z=z, stride=stride, pad=pad, relu=relu, **f), f['y'].reshape(z.shape)


def bottleneck_stage_batch(x, blocks, stats, g_out=None, eps=EPS):
    """torchvision's Bottleneck (stride on conv2) with every BatchNorm in training mode, gamma = c['scale'], beta = c['shift'];
    ``stats`` = per block {c1, c2, c3[, ds]: dict(running_mean, running_var, f)} -> dict(out, pres, running = the updated statistics in
    the order block by block c1, c2, c3[, ds]) and, with g_out, g_x, g_w, g_gamma, g_beta in that order."""
    tape, pres, running = [], [], []
    for blk, st in zip(blocks, stats):
        s = blk['stride']
        r1, y1 = _conv_bn(x, blk['c1'], 1, 0, st['c1'], eps)
        r2, y2 = _conv_bn(y1, blk['c2'], s, 1, st['c2'], eps)
        rd, idn = (None, x)
        if 'ds' in blk:
            rd, idn = _conv_bn(x, blk['ds'], s, 0, st['ds'], eps, relu=False)
        r3, out = _conv_bn(y2, blk['c3'], 1, 0, st['c3'], eps, res=idn)
        recs = [r1, r2, r3] + ([rd] if rd is not None else [])
        tape.append(recs)
        pres += [r['pre'] for r in recs if r['relu']]
        running += [(r['running_mean'], r['running_var']) for r in recs]
        x = out
    res = dict(out=x, pres=pres, running=running)
    if g_out is None:
        return res

    def bwd(rec, c, g_y, g_x_add=None):
        C = rec['z'].shape[-1]
        g_z, g_gamma, g_beta, g_res = backward(rec['z'].reshape(-1, C), c['scale'], rec['mean'], rec['invstd'], rec['pre'], g_y.reshape(-1, C), rec['relu'])
        g_x, g_w, _ = R.layer_backward(rec['x'], c['w'], torch.ones_like(c['scale']), rec['stride'], rec['pad'], None, g_z.reshape(rec['z'].shape),
                                       False, g_x_add)
        return g_x, g_w, g_gamma, g_beta, g_res.reshape(rec['z'].shape)
    g, g_w, g_gamma, g_beta = g_out, [], [], []
    for blk, recs in zip(reversed(blocks), reversed(tape)):
        g_y2, w3, ga3, be3, g_res = bwd(recs[2], blk['c3'], g)
        skip, extra = g_res, []
        if 'ds' in blk:
            skip, wd, gad, bed, _ = bwd(recs[3], blk['ds'], g_res)
            extra = [(wd, gad, bed)]
        g_y1, w2, ga2, be2, _ = bwd(recs[1], blk['c2'], g_y2)
        g, w1, ga1, be1, _ = bwd(recs[0], blk['c1'], g_y1, skip)
        grads = [(w1, ga1, be1), (w2, ga2, be2), (w3, ga3, be3)] + extra
        g_w = [t[0] for t in grads] + g_w
        g_gamma = [t[1] for t in grads] + g_gamma
        g_beta = [t[2] for t in grads] + g_beta
    res.update(g_x=g, g_w=g_w, g_gamma=g_gamma, g_beta=g_beta)
    return res


STAGE = dict(inplanes=16, planes=8, nblocks=2, stride=2, B=2, H=5, W=6)
MOMENTUM = 0.1


def _stage_stats(seed, blocks):
    g = torch.Generator().manual_seed(seed + 500)
    stats = []
    for blk in blocks:
        st = {}
        for c in ('c1', 'c2', 'c3', 'ds'):
            if c in blk:
                n = blk[c]['w'].shape[0]
                st[c] = dict(running_mean=_f32(0.2 * torch.randn(n, generator=g, dtype=torch.float64)),
                             running_var=_f32(0.5 + torch.rand(n, generator=g, dtype=torch.float64)), f=MOMENTUM)
        stats.append(st)
    return stats


def stage_case(base_seed=0):
    """The small stage of tests/test_gpu_stage_batchnorm.py: planes 8, two blocks, the first with stride 2 and a downsample, B = 2, a
    5 x 6 input; seven conv weights and seven BatchNorms with random running statistics.  The seed walks upward until the mask
    condition holds for every BatchNorm followed by a ReLU."""
    for step in range(64):
        t = R._stage_tensors(base_seed + step, **STAGE)
        t['x'], t['g_out'] = _f32(t['x']), _f32(t['g_out'])
        for blk in t['blocks']:
            for c in ('c1', 'c2', 'c3', 'ds'):
                if c in blk:
                    blk[c] = {k: _f32(v) for k, v in blk[c].items()}
        t['stats'] = _stage_stats(base_seed + step, t['blocks'])
        if R.band_empty(bottleneck_stage_batch(t['x'], t['blocks'], t['stats'])['pres']):
            t.update(seed=base_seed + step, seed_steps=step)
            return t
    raise RuntimeError('no seed with an empty band for the stage case')


def stage_module(case_, dtype=torch.float32):
    """The blocks of a stage case as the trunk's own parameter containers (``spec_amd.modules._BottleneckParams``), in ``train()``:
    gamma = scale, beta = shift, the case's running statistics and momentum."""
    import torch.nn as nn
    from spec_amd.modules import _BottleneckParams
    blocks = []
    for b, st in zip(case_['blocks'], case_['stats']):
        planes, inplanes = b['c1']['w'].shape[:2]
        m = _BottleneckParams(inplanes, planes, b['stride'], 'ds' in b)
        pairs = [(m.conv1, m.bn1, 'c1'), (m.conv2, m.bn2, 'c2'), (m.conv3, m.bn3, 'c3')] + ([(m.downsample[0], m.downsample[1], 'ds')] if 'ds' in b else [])
        with torch.no_grad():
            for conv, bn, c in pairs:
                conv.weight.copy_(b[c]['w'])
                bn.weight.copy_(b[c]['scale']); bn.bias.copy_(b[c]['shift'])
                bn.running_mean.copy_(st[c]['running_mean']); bn.running_var.copy_(st[c]['running_var'])
                bn.momentum, bn.eps = st[c]['f'], EPS
        blocks.append(m)
    return nn.Sequential(*blocks).to(dtype).train()


def torch_stage(mods, x):
    """torch's own chain on the containers of ``stage_module`` in whatever mode they are in: ``F.conv2d`` and the BatchNorm modules
    themselves (batch statistics and the running-statistics update in ``train()``); x NHWC -> NHWC."""
    v = x.permute(0, 3, 1, 2)
    for m in mods:
        y = torch.relu(m.bn1(m.conv1(v)))
        y = torch.relu(m.bn2(m.conv2(y)))
        idn = m.downsample(v) if hasattr(m, 'downsample') else v
        v = torch.relu(m.bn3(m.conv3(y)) + idn)
    return v.permute(0, 2, 3, 1)


def module_bns(mods):
    return [bn for m in mods for bn in [m.bn1, m.bn2, m.bn3] + ([m.downsample[1]] if hasattr(m, 'downsample') else [])]


# ---- six steps of gradient descent on the stage, its gammas and betas, and three linear heads -----------------------------------
SGD_STEPS, SGD_NBINS = R.SGD_STEPS, R.SGD_NBINS
# chosen on the float64 chain below so that the loss falls at every one of the six steps at this rate AND at twice it
# (tests/test_bn_ref_host.py asserts both) - the factor-2 margin the device run is given
SGD_RATE = 0.02


def sgd_problem():
    """The stage case with three one-Linear heads (N(0, 0.05) weights, zero bias) on the pooled output and cross-entropy targets."""
    t = stage_case()
    g = torch.Generator().manual_seed(98)
    F_ = t['blocks'][-1]['c3']['w'].shape[0]
    head = {}
    for k in ('fc_vfov', 'fc_pitch', 'fc_roll'):
        head[k + '.weight'] = _f32(0.05 * torch.randn(SGD_NBINS, F_, generator=g, dtype=torch.float64))
        head[k + '.bias'] = torch.zeros(SGD_NBINS, dtype=torch.float64)
    return dict(stage=t, head=head, targets=torch.randint(0, SGD_NBINS, (3, t['x'].shape[0]), generator=g))


def sgd_losses64(rate=SGD_RATE, steps=SGD_STEPS):
    """The losses of ``steps`` steps of plain gradient descent on the seven conv weights, the seven gammas and betas and the six head
    tensors, in float64 with torch's own autograd on ``F.conv2d`` and BatchNorm modules in ``train()``: steps + 1 values (the last
    one is one more training-mode forward).  loss = the sum over the heads of the mean cross-entropy."""
    import torch.nn.functional as F
    p = sgd_problem()
    mods = stage_module(p['stage'], torch.float64)
    head = {k: v.clone().requires_grad_(True) for k, v in p['head'].items()}
    leaves = list(mods.parameters()) + list(head.values())

    def loss_of():
        xf = torch_stage(mods, p['stage']['x']).mean(dim=(1, 2))
        return sum(F.cross_entropy(xf @ head[k + '.weight'].T + head[k + '.bias'], p['targets'][j]) for j, k in enumerate(('fc_vfov', 'fc_pitch', 'fc_roll')))
    losses = []
    with torch.enable_grad():
        for _ in range(steps):
            loss = loss_of()
            grads = torch.autograd.grad(loss, leaves)
            losses.append(float(loss.detach()))
            with torch.no_grad():
                for leaf, g in zip(leaves, grads):
                    leaf -= rate * g
        losses.append(float(loss_of().detach()))
    return losses
