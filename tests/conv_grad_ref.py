"""The float64 reference of the trainable ResNet layer (``specmi_conv2d_train_forward`` / ``specmi_conv2d_backward``,
spec_amd/csrc/conv_bwd.hip) and of a stage of bottlenecks (``spec_amd.differentiable.ResNetStage``), written directly - tap by
tap on strided slices, no ``F.conv2d``, no autograd - in torch CPU tensors of the dtype asked for (float64; float32 for the
exact cases, whose two evaluations must agree bit for bit).

The layer:  z = conv(x, w) * scale + shift [+ res],  y = relu ? max(z, 0) : z,  x / y / res NHWC, w OIHW.
Its backward, from g_y:  g_z = relu ? (z > 0 ? g_y : 0) : g_y  (the mask is taken from the reference's OWN pre-activation),
G = g_z * scale,  g_res = g_z,  g_x = conv^T(G, w) [+ g_x_add],  g_w = sum over the output pixels of G (x) the gathered x.

``err(a, b) = max|a - b| / max|b|``.

Mask condition (checked here, on the CPU): a float-valued case with relu is usable only if no float64 pre-activation z of any
layer lies within ``BAND * max|z|`` of zero, BAND = 2e-5 - twice the 1e-5 bound the forward value itself must meet, so a conforming
forward cannot flip a mask bit.  The generators walk seeds upward from their base until the band is empty and report the number
of steps; tests/test_conv_grad_ref_host.py asserts every committed case finds one within 16 seeds.

Exact cases: inputs, weights and gradients are small integers, scale in {0.5, 1, 2} and shift an integer, so every sum is exact
in fp32 and some z are exactly 0 (no gradient passes there).
"""
import numpy as np
import torch

BAND = 2e-5
MAX_SEED_STEPS = 16

# (B, H, W, Cin, Cout, k, stride): the smallest shapes at which each mechanism of the kernels can fail
LAYER_CASES = [
    (2, 5, 7, 33, 35, 1, 1),      # tails everywhere, three row tiles
    (2, 5, 7, 33, 35, 1, 2),      # odd extents; input pixels no tap reaches must get exactly 0
    (1, 1, 1, 40, 33, 3, 1),      # the centre tap alone
    (2, 3, 3, 9, 34, 3, 1),       # every pixel touches padding
    (2, 6, 5, 33, 32, 3, 2),      # even and odd extents at stride 2
    (3, 4, 4, 130, 3, 3, 1),      # k past one trip of every wave with a tail, Cout < 32
    (33, 1, 1, 8, 8, 1, 1),       # rows crossing a tile, wgrad contraction of 33
]


def err(a, b):
    a = torch.as_tensor(a).detach().cpu().double()
    b = torch.as_tensor(b).detach().cpu().double()
    den = b.abs().max().item()
    return (a - b).abs().max().item() / (den if den > 0 else 1.0)


def out_size(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def _taps(x, k, stride, pad, OH, OW):
    """x (B, H, W, C) -> yields (ky, kx, the (B, OH, OW, C) view of the zero-padded x that tap reads)."""
    B, H, W, C = x.shape
    xp = x.new_zeros(B, H + 2 * pad, W + 2 * pad, C)
    xp[:, pad:pad + H, pad:pad + W] = x
    for ky in range(k):
        for kx in range(k):
            yield ky, kx, xp[:, ky:ky + (OH - 1) * stride + 1:stride, kx:kx + (OW - 1) * stride + 1:stride]


def layer_forward(x, w, scale, shift, stride, pad, res=None, relu=True):
    """-> (y, z): the layer's output and its pre-activation, in x's dtype."""
    B, H, W, _ = x.shape
    Cout, _, k, _ = w.shape
    OH, OW = out_size(H, k, stride, pad), out_size(W, k, stride, pad)
    acc = x.new_zeros(B, OH, OW, Cout)
    for ky, kx, patch in _taps(x, k, stride, pad, OH, OW):
        acc = acc + torch.einsum('bhwc,oc->bhwo', patch, w[:, :, ky, kx])
    z = acc * scale + shift
    if res is not None:
        z = z + res
    return (z.clamp_min(0) if relu else z), z


def layer_backward(x, w, scale, stride, pad, z, g_y, relu=True, g_x_add=None):
    """-> (g_x, g_w, g_res); z = the pre-activation ``layer_forward`` returned (read only with relu)."""
    B, H, W, Cin = x.shape
    Cout, _, k, _ = w.shape
    OH, OW = out_size(H, k, stride, pad), out_size(W, k, stride, pad)
    g_z = torch.where(z > 0, g_y, torch.zeros_like(g_y)) if relu else g_y
    G = g_z * scale
    g_w = torch.zeros_like(w)
    g_xp = x.new_zeros(B, H + 2 * pad, W + 2 * pad, Cin)
    for ky, kx, patch in _taps(x, k, stride, pad, OH, OW):
        g_w[:, :, ky, kx] = torch.einsum('bhwo,bhwc->oc', G, patch)
        g_xp[:, ky:ky + (OH - 1) * stride + 1:stride, kx:kx + (OW - 1) * stride + 1:stride] += torch.einsum('bhwo,oc->bhwc', G, w[:, :, ky, kx])
    g_x = g_xp[:, pad:pad + H, pad:pad + W].clone()
    if g_x_add is not None:
        g_x = g_x + g_x_add
    return g_x, g_w, g_z


def band_empty(zs):
    """The mask condition: no element of any pre-activation within BAND * max|z| of zero."""
    return all(z.abs().min().item() > BAND * z.abs().max().item() for z in zs)


def _layer_tensors(shape, seed, exact):
    B, H, W, Cin, Cout, k, stride = shape
    pad = k // 2
    OH, OW = out_size(H, k, stride, pad), out_size(W, k, stride, pad)
    g = torch.Generator().manual_seed(seed)
    if exact:
        def ints(lo, hi, *s):
            return torch.randint(lo, hi + 1, s, generator=g).double()
        t = dict(x=ints(-3, 3, B, H, W, Cin), w=ints(-2, 2, Cout, Cin, k, k), scale=torch.tensor([0.5, 1.0, 2.0]).double()[torch.randint(0, 3, (Cout,), generator=g)],
                 shift=ints(-2, 2, Cout), res=ints(-3, 3, B, OH, OW, Cout), g_y=ints(-3, 3, B, OH, OW, Cout), g_x_add=ints(-3, 3, B, H, W, Cin))
    else:
        def rn(*s):
            return torch.randn(*s, generator=g, dtype=torch.float64)
        t = dict(x=rn(B, H, W, Cin), w=rn(Cout, Cin, k, k) / float(np.sqrt(Cin * k * k)), scale=0.5 + torch.rand(Cout, generator=g, dtype=torch.float64),
                 shift=0.5 * rn(Cout), res=rn(B, OH, OW, Cout), g_y=rn(B, OH, OW, Cout), g_x_add=rn(B, H, W, Cin))
    t.update(stride=stride, pad=pad, shape=shape)
    return t


def layer_case(shape, base_seed=0, exact=False):
    """The tensors of one layer case (float64) with ``seed`` and ``seed_steps``.  A float-valued case satisfies the mask condition
    with and without the residual; an exact one is taken at its base seed (z == 0 is what it is for)."""
    for step in range(64):
        t = _layer_tensors(shape, base_seed + step, exact)
        if exact:
            # every fifth pre-activation (with the residual) is made exactly 0 through the residual, which stays a multiple of 0.5
            z = layer_forward(t['x'], t['w'], t['scale'], t['shift'], t['stride'], t['pad'], t['res'], True)[1]
            hit = (torch.arange(z.numel()) % 5 == 0).view(z.shape)
            t['res'] = torch.where(hit, t['res'] - z, t['res'])
            break
        zs = [layer_forward(t['x'], t['w'], t['scale'], t['shift'], t['stride'], t['pad'], res, True)[1] for res in (None, t['res'])]
        if band_empty(zs):
            break
    else:
        raise RuntimeError(f'no seed with an empty band for {shape}')
    t.update(seed=base_seed + step, seed_steps=step)
    return t


# ---- a stage of bottlenecks -------------------------------------------------------------------------------------------------
def _stage_tensors(seed, inplanes, planes, nblocks, stride, B, H, W):
    g = torch.Generator().manual_seed(seed)

    def rn(*s):
        return torch.randn(*s, generator=g, dtype=torch.float64)

    def conv(cout, cin, k):
        return dict(w=rn(cout, cin, k, k) / float(np.sqrt(cin * k * k)), scale=0.5 + torch.rand(cout, generator=g, dtype=torch.float64), shift=0.3 * rn(cout))
    blocks = []
    cin = inplanes
    for i in range(nblocks):
        s = stride if i == 0 else 1
        blk = dict(stride=s, c1=conv(planes, cin, 1), c2=conv(planes, planes, 3), c3=conv(4 * planes, planes, 1))
        if i == 0 and (s != 1 or cin != 4 * planes):
            blk['ds'] = conv(4 * planes, cin, 1)
        blocks.append(blk)
        cin = 4 * planes
    OH, OW = out_size(H, 3, stride, 1), out_size(W, 3, stride, 1)
    return dict(x=rn(B, H, W, inplanes), blocks=blocks, g_out=rn(B, OH, OW, 4 * planes))


def bottleneck_stage(x, blocks, g_out=None):
    """torchvision's Bottleneck (stride on conv2) on frozen BatchNorm, block after block -> dict(out, zs) and, with g_out, g_x and
    g_w = the weight gradients in the order block by block conv1, conv2, conv3[, downsample]."""
    tape, zs = [], []
    for blk in blocks:
        c1, c2, c3, s = blk['c1'], blk['c2'], blk['c3'], blk['stride']
        y1, z1 = layer_forward(x, c1['w'], c1['scale'], c1['shift'], 1, 0)
        y2, z2 = layer_forward(y1, c2['w'], c2['scale'], c2['shift'], s, 1)
        idn = x
        if 'ds' in blk:
            idn, _ = layer_forward(x, blk['ds']['w'], blk['ds']['scale'], blk['ds']['shift'], s, 0, relu=False)
        out, z3 = layer_forward(y2, c3['w'], c3['scale'], c3['shift'], 1, 0, res=idn)
        tape.append((x, y1, z1, y2, z2, z3))
        zs += [z1, z2, z3]
        x = out
    r = dict(out=x, zs=zs)
    if g_out is None:
        return r
    g, g_w = g_out, []
    for blk, (xin, y1, z1, y2, z2, z3) in zip(reversed(blocks), reversed(tape)):
        c1, c2, c3, s = blk['c1'], blk['c2'], blk['c3'], blk['stride']
        g_y2, gw3, g_res = layer_backward(y2, c3['w'], c3['scale'], 1, 0, z3, g)
        skip, gwd = g_res, None
        if 'ds' in blk:
            skip, gwd, _ = layer_backward(xin, blk['ds']['w'], blk['ds']['scale'], s, 0, None, g_res, relu=False)
        g_y1, gw2, _ = layer_backward(y1, c2['w'], c2['scale'], s, 1, z2, g_y2)
        g, gw1, _ = layer_backward(xin, c1['w'], c1['scale'], 1, 0, z1, g_y1, g_x_add=skip)
        g_w = [gw1, gw2, gw3] + ([gwd] if gwd is not None else []) + g_w
    r.update(g_x=g, g_w=g_w)
    return r


def stage_case(base_seed=0, inplanes=64, planes=32, nblocks=3, stride=2, B=2, H=5, W=6):
    """The synthetic stage of tests/test_gpu_trunk_finetune.py (float64): planes 32, three blocks, the first with stride 2 and a
    downsample, B = 2, a 5 x 6 input; ten conv weights.  The seed walks upward until the mask condition holds for every layer."""
    for step in range(64):
        t = _stage_tensors(base_seed + step, inplanes, planes, nblocks, stride, B, H, W)
        if band_empty(bottleneck_stage(t['x'], t['blocks'])['zs']):
            t.update(seed=base_seed + step, seed_steps=step)
            return t
    raise RuntimeError('no seed with an empty band for the stage case')


# ---- six steps of gradient descent on a stage and three linear heads ------------------------------------------------------------
SGD_STEPS, SGD_NBINS = 6, 16
# chosen on the float64 chain below so that the loss falls at every one of the six steps at this rate AND at twice it
# (tests/test_conv_grad_ref_host.py asserts both) - the factor-2 margin the device run is given
SGD_RATE = 0.01


def sgd_problem():
    """The stage case with three one-Linear heads (N(0, 0.05) weights, zero bias) on the pooled output and cross-entropy targets:
    -> dict(stage = ``stage_case()``, head = {fc_vfov.weight, ...} float64, targets (3, B) int64)."""
    t = stage_case()
    g = torch.Generator().manual_seed(97)
    F_ = t['blocks'][-1]['c3']['w'].shape[0]
    head = {}
    for k in ('fc_vfov', 'fc_pitch', 'fc_roll'):
        head[k + '.weight'] = 0.05 * torch.randn(SGD_NBINS, F_, generator=g, dtype=torch.float64)
        head[k + '.bias'] = torch.zeros(SGD_NBINS, dtype=torch.float64)
    return dict(stage=t, head=head, targets=torch.randint(0, SGD_NBINS, (3, t['x'].shape[0]), generator=g))


def sgd_losses64(rate=SGD_RATE, steps=SGD_STEPS):
    """The losses of ``steps`` steps of plain gradient descent on the ten conv weights and the six head tensors, in float64 with
    torch's own autograd on ``F.conv2d`` (BatchNorm frozen): steps + 1 values.  loss = the sum over the heads of the mean
    cross-entropy (``CameraRegressorLoss(1, 1, 1, 'ce')``)."""
    import torch.nn.functional as F
    p = sgd_problem()
    blocks = p['stage']['blocks']
    names = [(i, c) for i, b in enumerate(blocks) for c in ('c1', 'c2', 'c3', 'ds') if c in b]
    leaves = [blocks[i][c]['w'].clone().requires_grad_(True) for i, c in names] + [v.clone().requires_grad_(True) for v in p['head'].values()]

    def loss_of():
        w = dict(zip(names, leaves))
        hp = dict(zip(p['head'], leaves[len(names):]))

        def layer(v, i, c, s, pad, relu, res=None):
            z = F.conv2d(v.permute(0, 3, 1, 2), w[(i, c)], stride=s, padding=pad).permute(0, 2, 3, 1) * blocks[i][c]['scale'] + blocks[i][c]['shift']
            z = z if res is None else z + res
            return torch.relu(z) if relu else z
        v = p['stage']['x']
        for i, b in enumerate(blocks):
            y2 = layer(layer(v, i, 'c1', 1, 0, True), i, 'c2', b['stride'], 1, True)
            v = layer(y2, i, 'c3', 1, 0, True, layer(v, i, 'ds', b['stride'], 0, False) if 'ds' in b else v)
        xf = v.mean(dim=(1, 2))
        return sum(F.cross_entropy(xf @ hp[k + '.weight'].T + hp[k + '.bias'], p['targets'][j]) for j, k in enumerate(('fc_vfov', 'fc_pitch', 'fc_roll')))
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
