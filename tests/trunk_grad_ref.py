"""The float64 references of what the trainable trunk adds below the bottleneck stages: MaxPool2d(3, 2, 1) with the record of the
winning tap and its gradient (``specmi_maxpool3x3s2_train_forward`` / ``specmi_maxpool3x3s2_backward``, spec_amd/csrc/pool_bwd.hip),
and the stem chain conv7x7/2 -> scale / shift -> ReLU -> max-pool built on tests/conv_grad_ref.py's ``layer_forward`` /
``layer_backward``, which are generic in k.  Written directly - no ``F.max_pool2d``, no autograd - in torch CPU tensors of the
dtype given; tests/test_trunk_grad_ref_host.py pins them to torch's own float64 autograd.

Max-pool, torch's rule: the in-range taps of a window are scanned in (ky, kx) ascending order, a tap replaces the best so far when
``v > best or isnan(v)``; ``idx = ky * 3 + kx`` of the tap the scan ends on (the first in-range tap where nothing replaced -inf).
Its backward: g_x[pixel] = the sum of g_y over the windows whose idx names the pixel, added in (oy, ox) ascending order.

Mask condition of a float case that has a pool behind a convolution (it extends ``conv_grad_ref.band_empty``): no pre-activation
within the band of zero, AND in every pool window the two largest values are bit-equal or differ by more than BAND * max|x| - a
forward inside its bound can then not move a window's winner.
"""
import torch

from tests import conv_grad_ref as R

BAND = R.BAND
MAX_SEED_STEPS = 64
err = R.err

# (B, H, W, C) of tests/test_gpu_maxpool_backward.py
POOL_CASES = [(1, 1, 1, 1), (1, 2, 2, 4), (2, 5, 7, 5), (2, 6, 4, 64), (1, 7, 9, 68)]
# (B, H, W, Cin, Cout, k, stride) of tests/test_gpu_stem_backward.py: conv_grad_ref.layer_case takes pad = k // 2 = 3
STEM_CASES = [(2, 9, 11, 3, 5, 7, 2), (1, 1, 1, 3, 33, 7, 2), (1, 7, 7, 3, 64, 7, 2), (2, 16, 13, 3, 64, 7, 2), (1, 6, 5, 4, 9, 7, 2)]


def pool_size(n):
    return (n - 1) // 2 + 1


def _pool_taps(H, W):
    OH, OW = pool_size(H), pool_size(W)
    for ky in range(3):
        for kx in range(3):
            yield ky * 3 + kx, slice(ky, ky + 2 * (OH - 1) + 1, 2), slice(kx, kx + 2 * (OW - 1) + 1, 2)


def maxpool_forward(x):
    """x (B, H, W, C) -> (y (B, OH, OW, C) in x's dtype, idx uint8)."""
    B, H, W, C = x.shape
    xp = x.new_full((B, H + 2, W + 2, C), float('-inf'))
    xp[:, 1:H + 1, 1:W + 1] = x
    inside = torch.zeros(1, H + 2, W + 2, 1, dtype=torch.bool)
    inside[:, 1:H + 1, 1:W + 1] = True
    OH, OW = pool_size(H), pool_size(W)
    best = x.new_full((B, OH, OW, C), float('-inf'))
    idx = torch.full((B, OH, OW, C), 255, dtype=torch.uint8)
    for k, sy, sx in _pool_taps(H, W):
        v, ok = xp[:, sy, sx], inside[:, sy, sx].expand(B, OH, OW, C)
        idx = torch.where(ok & (idx == 255), torch.full_like(idx, k), idx)          # where torch's scan starts
        take = ok & ((v > best) | torch.isnan(v))
        best = torch.where(take, v, best)
        idx = torch.where(take, torch.full_like(idx, k), idx)
    return best, idx


def maxpool_backward(g_y, idx, H, W):
    """-> g_x (B, H, W, C) in g_y's dtype.  The taps are walked in DESCENDING order: a pixel meets its windows in (oy, ox) ascending
    order then (window oy reaches row iy through tap ky = iy + 1 - 2 oy)."""
    B, OH, OW, C = g_y.shape
    g = g_y.new_zeros(B, H + 2, W + 2, C)
    for k, sy, sx in reversed(list(_pool_taps(H, W))):
        g[:, sy, sx] += torch.where(idx == k, g_y, torch.zeros_like(g_y))
    return g[:, 1:H + 1, 1:W + 1].clone()


def pool_band_empty(x):
    """In every window of x (B, H, W, C) the two largest in-range values are bit-equal or more than BAND * max|x| apart."""
    B, H, W, C = x.shape
    xp = x.new_full((B, H + 2, W + 2, C), float('-inf'))
    xp[:, 1:H + 1, 1:W + 1] = x
    top = torch.stack([xp[:, sy, sx] for _, sy, sx in _pool_taps(H, W)]).sort(0, descending=True).values
    a, b = top[0], top[1]
    return bool(((a == b) | (a - b > BAND * x.abs().max())).all())


# ---- the stem chain on a frozen BatchNorm ---------------------------------------------------------------------------------------
def stem_forward(x, w, scale, shift):
    """x (B, H, W, Cin) NHWC -> dict(out = pool(relu(conv7x7/2(x) scale + shift)), y, z, idx)."""
    y, z = R.layer_forward(x, w, scale, shift, 2, 3)
    out, idx = maxpool_forward(y)
    return dict(out=out, y=y, z=z, idx=idx)


def stem_backward(x, w, scale, f, g_out):
    """f = ``stem_forward``'s dict -> g_w; the images get no gradient."""
    g_y = maxpool_backward(g_out, f['idx'], f['y'].shape[1], f['y'].shape[2])
    return R.layer_backward(x, w, scale, 2, 3, f['z'], g_y)[1]


def stem_case(shape=(2, 33, 29, 3, 8), base_seed=0):
    """(B, H, W, Cin, Cout) -> the tensors of a stem case, float64 holding fp32 values, whose seed walks upward until the mask
    condition holds: the band of zero empty and every pool window decided."""
    B, H, W, Cin, Cout = shape
    for step in range(MAX_SEED_STEPS):
        g = torch.Generator().manual_seed(base_seed + step)
        rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float().double()
        t = dict(x=rn(B, H, W, Cin), w=(rn(Cout, Cin, 7, 7) / float((Cin * 49) ** 0.5)).float().double(),
                 scale=(0.5 + torch.rand(Cout, generator=g, dtype=torch.float64)).float().double(), shift=0.3 * rn(Cout))
        t['shift'] = t['shift'].float().double()
        f = stem_forward(t['x'], t['w'], t['scale'], t['shift'])
        t['g_out'] = rn(*f['out'].shape)
        if R.band_empty([f['z']]) and pool_band_empty(f['y']):
            t.update(seed=base_seed + step, seed_steps=step, shape=shape)
            return t
    raise RuntimeError(f'no seed with the mask condition for {shape}')


# ---- a small whole trunk: stem 3 -> 8, one bottleneck per stage with planes 8 / 8 / 16 / 16 ---------------------------------------
TRUNK = dict(B=2, H=33, W=29, stem=8, planes=(8, 8, 16, 16), strides=(1, 2, 2, 2))
MOMENTUM = 0.1


def _fold(c, st, eps):
    """gamma / beta / running statistics -> the frozen affine map, in float64."""
    scale = c['scale'] / torch.sqrt(st['running_var'] + eps)
    return dict(w=c['w'], scale=scale, shift=c['shift'] - st['running_mean'] * scale)


def trunk_frozen(t, g_out=None, eps=1e-5):
    """The small trunk on FROZEN BatchNorm (every BN folded from its running statistics) -> dict(out, zs, y = the stem's
    activation) and, with g_out, g_w = [the stem's, then block by block conv1, conv2, conv3, downsample]."""
    s = _fold(t['stem'], t['stem_stat'], eps)
    blocks = [dict(stride=b['stride'], **{c: _fold(b[c], st[c], eps) for c in ('c1', 'c2', 'c3', 'ds') if c in b})
              for b, st in zip(t['blocks'], t['stats'])]
    f = stem_forward(t['x'], s['w'], s['scale'], s['shift'])
    r = R.bottleneck_stage(f['out'], blocks, g_out)
    res = dict(out=r['out'], zs=[f['z']] + r['zs'], y=f['y'])
    if g_out is not None:
        res['g_w'] = [stem_backward(t['x'], s['w'], s['scale'], f, r['g_x'])] + r['g_w']
    return res


def trunk_batch(t, g_out=None, eps=1e-5):
    """The small trunk with every BatchNorm in training mode (tests/bn_ref.py's formulas) -> dict(out, pres, y, running) and, with
    g_out, g_w, g_gamma, g_beta, the stem's first."""
    from tests import bn_ref as N
    c, st = t['stem'], t['stem_stat']
    ones, zeros = torch.ones_like(c['scale']), torch.zeros_like(c['shift'])
    z = R.layer_forward(t['x'], c['w'], ones, zeros, 2, 3, None, False)[0]
    C = z.shape[-1]
    f = N.forward(z.reshape(-1, C), c['scale'], c['shift'], eps, None, True, st['running_mean'], st['running_var'], st['f'])
    y = f['y'].reshape(z.shape)
    out, idx = maxpool_forward(y)
    r = N.bottleneck_stage_batch(out, t['blocks'], t['stats'], g_out, eps)
    res = dict(out=r['out'], pres=[f['pre']] + r['pres'], y=y, running=[(f['running_mean'], f['running_var'])] + r['running'])
    if g_out is not None:
        g_y = maxpool_backward(r['g_x'], idx, y.shape[1], y.shape[2])
        g_z, g_gamma, g_beta, _ = N.backward(z.reshape(-1, C), c['scale'], f['mean'], f['invstd'], f['pre'], g_y.reshape(-1, C), True)
        g_w = R.layer_backward(t['x'], c['w'], ones, 2, 3, None, g_z.reshape(z.shape), False)[1]
        res.update(g_w=[g_w] + r['g_w'], g_gamma=[g_gamma] + r['g_gamma'], g_beta=[g_beta] + r['g_beta'])
    return res


def trunk_case(base_seed=0):
    """The tensors of the small trunk, float64 holding fp32 values: x NHWC images, stem / blocks = dict(w, scale = gamma, shift =
    beta), stem_stat / stats = dict(running_mean, running_var, f), g_out.  The seed walks upward until the mask condition holds on
    the frozen AND the batch chain: every pre-activation's band of zero empty, every window of the stem's pool decided."""
    f32 = lambda v: v.float().double()
    B, H, W = TRUNK['B'], TRUNK['H'], TRUNK['W']
    for step in range(MAX_SEED_STEPS):
        seed = base_seed + step
        g = torch.Generator().manual_seed(seed)
        rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
        stat = lambda n: dict(running_mean=f32(0.2 * rn(n)), running_var=f32(0.5 + torch.rand(n, generator=g, dtype=torch.float64)), f=MOMENTUM)
        c0 = TRUNK['stem']
        t = dict(x=f32(rn(B, H, W, 3)), stem=dict(w=f32(rn(c0, 3, 7, 7) / 147 ** 0.5), scale=f32(0.5 + torch.rand(c0, generator=g, dtype=torch.float64)),
                                                   shift=f32(0.3 * rn(c0))), stem_stat=stat(c0), blocks=[], stats=[])
        cin = c0
        for i, (planes, stride) in enumerate(zip(TRUNK['planes'], TRUNK['strides'])):
            blk = R._stage_tensors(1000 * seed + i, cin, planes, 1, stride, 1, 1, 1)['blocks'][0]
            blk = {k: ({kk: f32(vv) for kk, vv in v.items()} if isinstance(v, dict) else v) for k, v in blk.items()}
            t['blocks'].append(blk)
            t['stats'].append({c: stat(blk[c]['w'].shape[0]) for c in ('c1', 'c2', 'c3', 'ds') if c in blk})
            cin = 4 * planes
        fr, ba = trunk_frozen(t), trunk_batch(t)
        t['g_out'] = f32(rn(*fr['out'].shape))
        if R.band_empty(fr['zs']) and R.band_empty(ba['pres']) and pool_band_empty(fr['y']) and pool_band_empty(ba['y']):
            t.update(seed=seed, seed_steps=step)
            return t
    raise RuntimeError('no seed with the mask condition for the trunk case')


def trunk_modules(t, dtype=torch.float32):
    """The small trunk as the library's own parameter containers -> (conv1, bn1, [one nn.Sequential of blocks per stage]), in
    ``train()``, with the case's gammas, betas, running statistics and momentum."""
    import torch.nn as nn
    from tests import bn_ref as N
    c, st = t['stem'], t['stem_stat']
    conv1, bn1 = nn.Conv2d(3, c['w'].shape[0], 7, stride=2, padding=3, bias=False), nn.BatchNorm2d(c['w'].shape[0])
    with torch.no_grad():
        conv1.weight.copy_(c['w'])
        bn1.weight.copy_(c['scale']); bn1.bias.copy_(c['shift'])
        bn1.running_mean.copy_(st['running_mean']); bn1.running_var.copy_(st['running_var'])
    bn1.momentum, bn1.eps = st['f'], N.EPS
    stages = [N.stage_module(dict(blocks=[b], stats=[s]), dtype) for b, s in zip(t['blocks'], t['stats'])]
    return conv1.to(dtype).train(), bn1.to(dtype).train(), stages


def torch_trunk(conv1, bn1, stages, x):
    """torch's own chain on the containers of ``trunk_modules`` in whatever mode they are in; x NHWC images -> NHWC."""
    import torch.nn.functional as F
    from tests import bn_ref as N
    v = F.max_pool2d(torch.relu(bn1(conv1(x.permute(0, 3, 1, 2)))), 3, 2, 1).permute(0, 2, 3, 1)
    for st in stages:
        v = N.torch_stage(st, v)
    return v


# ---- six steps of gradient descent on the small trunk and three linear heads ------------------------------------------------------
SGD_STEPS, SGD_NBINS = R.SGD_STEPS, R.SGD_NBINS
# chosen on the float64 chains below so that the loss falls at every one of the six steps at this rate AND at twice it, frozen and
# batch (tests/test_trunk_grad_ref_host.py asserts both) - the factor-2 margin the device run is given
SGD_RATE = 0.005


def sgd_problem():
    """The trunk case with three one-Linear heads (N(0, 0.05) weights, zero bias) on the pooled output and cross-entropy targets."""
    t = trunk_case()
    g = torch.Generator().manual_seed(99)
    F_ = t['blocks'][-1]['c3']['w'].shape[0]
    head = {}
    for k in ('fc_vfov', 'fc_pitch', 'fc_roll'):
        head[k + '.weight'] = (0.05 * torch.randn(SGD_NBINS, F_, generator=g, dtype=torch.float64)).float().double()
        head[k + '.bias'] = torch.zeros(SGD_NBINS, dtype=torch.float64)
    return dict(trunk=t, head=head, targets=torch.randint(0, SGD_NBINS, (3, t['x'].shape[0]), generator=g))


def sgd_losses64(bn='frozen', rate=SGD_RATE, steps=SGD_STEPS):
    """The losses of ``steps`` steps of plain gradient descent through ``trunk_frozen`` (the 17 conv weights) or ``trunk_batch`` (also
    the 17 gammas and betas, the running statistics moving) and the six head tensors, in float64: steps + 1 values.  Only the tail
    behind the trunk's output - the mean over the map, three Linear layers, the sum of the mean cross-entropies - goes through
    torch's autograd, which hands ``g_out`` to the chain."""
    import copy
    import torch.nn.functional as F
    p = sgd_problem()
    t = copy.deepcopy(p['trunk'])
    head = {k: v.clone() for k, v in p['head'].items()}
    chain = trunk_batch if bn == 'batch' else trunk_frozen
    convs = lambda: [t['stem']] + [b[c] for b in t['blocks'] for c in ('c1', 'c2', 'c3', 'ds') if c in b]
    stats = lambda: [t['stem_stat']] + [s[c] for b, s in zip(t['blocks'], t['stats']) for c in ('c1', 'c2', 'c3', 'ds') if c in b]

    def tail(out):
        leaf = out.clone().requires_grad_(True)
        hp = {k: v.clone().requires_grad_(True) for k, v in head.items()}
        with torch.enable_grad():
            xf = leaf.mean(dim=(1, 2))
            loss = sum(F.cross_entropy(xf @ hp[k + '.weight'].T + hp[k + '.bias'], p['targets'][j]) for j, k in enumerate(('fc_vfov', 'fc_pitch', 'fc_roll')))
            grads = torch.autograd.grad(loss, [leaf] + list(hp.values()))
        return float(loss.detach()), grads[0], dict(zip(hp, grads[1:]))
    losses = []
    for _ in range(steps):
        loss, g_out, g_head = tail(chain(t)['out'])
        r = chain(t, g_out)
        losses.append(loss)
        for c, g_w in zip(convs(), r['g_w']):
            c['w'] = c['w'] - rate * g_w
        if bn == 'batch':
            for c, st, gg, gb, (rm, rv) in zip(convs(), stats(), r['g_gamma'], r['g_beta'], r['running']):
                c['scale'], c['shift'] = c['scale'] - rate * gg, c['shift'] - rate * gb
                st['running_mean'], st['running_var'] = rm, rv
        for k in head:
            head[k] = head[k] - rate * g_head[k]
    losses.append(tail(chain(t)['out'])[0])
    return losses


def sgd_losses_torch32(bn='frozen', rate=SGD_RATE, steps=SGD_STEPS):
    """The same descent in torch's own fp32 CPU autograd on the containers of ``trunk_modules``: what an fp32 chain other than the
    library's makes of the problem.  On batch statistics it leaves the float64 path by 1.6e-3 within six steps (layer4's BatchNorms
    see 4 values per channel and the masks move with the weights), on frozen BatchNorm by 5e-7."""
    import torch.nn.functional as F
    p = sgd_problem()
    t = p['trunk']
    conv1, bn1, stages = trunk_modules(t)
    for m in [conv1, bn1] + stages:
        m.train(bn == 'batch')
    head = {k: v.float().clone().requires_grad_(True) for k, v in p['head'].items()}
    blocks = [b for st in stages for b in st]
    params = [conv1.weight] + [q for b in blocks for q in (b.conv1.weight, b.conv2.weight, b.conv3.weight, b.downsample[0].weight)]
    if bn == 'batch':
        params += [q for m in [bn1] + [m for b in blocks for m in (b.bn1, b.bn2, b.bn3, b.downsample[1])] for q in (m.weight, m.bias)]
    opt = torch.optim.SGD(params + list(head.values()), lr=rate)
    x = t['x'].float()

    def loss_of():
        xf = torch_trunk(conv1, bn1, stages, x).mean(dim=(1, 2))
        return sum(F.cross_entropy(xf @ head[k + '.weight'].T + head[k + '.bias'], p['targets'][j]) for j, k in enumerate(('fc_vfov', 'fc_pitch', 'fc_roll')))
    losses = []
    with torch.enable_grad():
        for _ in range(steps):
            opt.zero_grad()
            loss = loss_of()
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(float(loss_of()))
    return losses
