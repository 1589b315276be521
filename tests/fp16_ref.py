"""Test-side reference of the fp16 trunk ("fp16 trunk"): a float64 walk of a torchvision ResNet trunk that rounds at
exactly the contract's points and nowhere else.

  * the image is rounded to fp16 (round to nearest even);
  * every convolution uses weights fp16_rne(w * s), s = gamma / sqrt(var + eps) computed in fp32 as the library folds it, the
    product in float64; products and sums in float64; + the fp32 BN shift (+ the fp16 residual), ReLU, rounded to fp16;
  * a bottleneck's downsample branch is summed into conv3 before the one rounding (the library folds it into conv3's GEMM);
  * the max-pool is exact; the last convolution of layer4 is not rounded (the library stores it in fp32).

Only the accumulation differs from the library (float64 here, fp32 on the matrix cores), so the two agree up to the rare
fp16 rounding flip that a different accumulation order causes."""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5


def f16(a):
    """float64 -> nearest-even fp16 -> float64 (numpy rounds float64 to float16 directly: no double rounding)."""
    return np.asarray(a, dtype=np.float64).astype(np.float16).astype(np.float64)


def fold(sd, prefix, conv, bn):
    """(fp16-rounded folded OIHW weights as float64, fp32 shift as float64), the library's BatchNorm fold (commit.hip)."""
    w = np.asarray(sd[f'{prefix}{conv}.weight'], dtype=np.float32)
    g, b, m, v = (np.asarray(sd[f'{prefix}{bn}.{k}'], dtype=np.float32) for k in ('weight', 'bias', 'running_mean', 'running_var'))
    invstd = np.float32(1.0) / np.sqrt(v + np.float32(EPS))
    s = (invstd * g).astype(np.float32)
    shift = (b - m * s).astype(np.float32)
    return f16(w.astype(np.float64) * s.astype(np.float64)[:, None, None, None]), shift.astype(np.float64)


def conv64(x, w, stride, pad):
    return F.conv2d(torch.from_numpy(x), torch.from_numpy(w), stride=stride, padding=pad).numpy()


def conv32(x, w, stride, pad):
    """The same convolution with float32 products and sums (fp16 operands are exact in float32), returned as float64."""
    return F.conv2d(torch.from_numpy(x).float(), torch.from_numpy(w).float(), stride=stride, padding=pad).double().numpy()


def _layout(depth):
    basic = depth in (18, 34)
    nblocks = {18: (2, 2, 2, 2), 34: (3, 4, 6, 3), 50: (3, 4, 6, 3), 101: (3, 4, 23, 3), 152: (3, 8, 36, 3)}[depth]
    return basic, nblocks


def trunk(sd, images, prefix='backbone.', depth=50, acc='float64'):
    """images (B,3,H,W) float -> layer4 features (B,C,h,w) float64 under the fp16 contract.  acc='float32' runs every
    convolution's accumulation in float32 on the same fp16 operands (the epilogue stays in float64): the distance between the
    two walks is the size of the rounding flips that an accumulation of the device's precision causes."""
    conv64 = {'float64': globals()['conv64'], 'float32': conv32}[acc]
    basic, nblocks = _layout(depth)
    x = f16(images)
    w, sh = fold(sd, prefix, 'conv1', 'bn1')
    x = f16(np.maximum(conv64(x, w, 2, 3) + sh[None, :, None, None], 0.0))
    x = F.max_pool2d(torch.from_numpy(x), 3, 2, 1).numpy()
    nb_total = sum(nblocks)
    bi = 0
    for li, nb in enumerate(nblocks):
        for b in range(nb):
            bi += 1
            last = bi == nb_total
            stride = 2 if (b == 0 and li > 0) else 1
            p = f'layer{li + 1}.{b}.'
            rnd = (lambda a: a) if last else f16
            ds = f'{prefix}{p}downsample.0.weight' in sd
            if basic:
                w1, s1 = fold(sd, prefix, p + 'conv1', p + 'bn1')
                y = f16(np.maximum(conv64(x, w1, stride, 1) + s1[None, :, None, None], 0.0))
                if ds:
                    wd, sd_ = fold(sd, prefix, p + 'downsample.0', p + 'downsample.1')
                    idn = f16(conv64(x, wd, stride, 0) + sd_[None, :, None, None])
                else:
                    idn = x
                w2, s2 = fold(sd, prefix, p + 'conv2', p + 'bn2')
                x = rnd(np.maximum(conv64(y, w2, 1, 1) + s2[None, :, None, None] + idn, 0.0))
                continue
            w1, s1 = fold(sd, prefix, p + 'conv1', p + 'bn1')
            y = f16(np.maximum(conv64(x, w1, 1, 0) + s1[None, :, None, None], 0.0))
            w2, s2 = fold(sd, prefix, p + 'conv2', p + 'bn2')
            y = f16(np.maximum(conv64(y, w2, stride, 1) + s2[None, :, None, None], 0.0))
            w3, s3 = fold(sd, prefix, p + 'conv3', p + 'bn3')
            acc = conv64(y, w3, 1, 0)
            if ds:   # folded into conv3: one sum, one rounding; the two fp32 shifts are added in fp32
                wd, sd_ = fold(sd, prefix, p + 'downsample.0', p + 'downsample.1')
                acc = acc + conv64(x, wd, stride, 0)
                shift = (s3.astype(np.float32) + sd_.astype(np.float32)).astype(np.float64)
                x = rnd(np.maximum(acc + shift[None, :, None, None], 0.0))
            else:
                x = rnd(np.maximum(acc + s3[None, :, None, None] + x, 0.0))
    return x


def trunk_fp64(sd, images, prefix='backbone.', depth=50):
    """The same walk with no rounding at all (eval-mode BatchNorm in float64): what fp16 is compared against on CPU."""
    basic, nblocks = _layout(depth)

    def cbn(x, conv, bn, stride, pad):
        w = np.asarray(sd[f'{prefix}{conv}.weight'], dtype=np.float64)
        g, b, m, v = (np.asarray(sd[f'{prefix}{bn}.{k}'], dtype=np.float64) for k in ('weight', 'bias', 'running_mean', 'running_var'))
        s = g / np.sqrt(v + EPS)
        return conv64(x, w, stride, pad) * s[None, :, None, None] + (b - m * s)[None, :, None, None]
    x = np.asarray(images, dtype=np.float64)
    x = np.maximum(cbn(x, 'conv1', 'bn1', 2, 3), 0.0)
    x = F.max_pool2d(torch.from_numpy(x), 3, 2, 1).numpy()
    for li, nb in enumerate(nblocks):
        for b in range(nb):
            stride = 2 if (b == 0 and li > 0) else 1
            p = f'layer{li + 1}.{b}.'
            ds = f'{prefix}{p}downsample.0.weight' in sd
            idn = cbn(x, p + 'downsample.0', p + 'downsample.1', stride, 0) if ds else x
            if basic:
                y = np.maximum(cbn(x, p + 'conv1', p + 'bn1', stride, 1), 0.0)
                x = np.maximum(cbn(y, p + 'conv2', p + 'bn2', 1, 1) + idn, 0.0)
                continue
            y = np.maximum(cbn(x, p + 'conv1', p + 'bn1', 1, 0), 0.0)
            y = np.maximum(cbn(y, p + 'conv2', p + 'bn2', stride, 1), 0.0)
            x = np.maximum(cbn(y, p + 'conv3', p + 'bn3', 1, 0) + idn, 0.0)
    return x


# ---- per-layer helpers shared by tests/test_gpu_fp16.py and tests/test_gpu_fp16_shapes.py -----------------------------------
DEV = 'cuda:0'
_conv64 = conv64


def nchw_to_nhwc(a):
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1))


def _run_shape(eng, cin, cout, k, stride, pad, H, W, B, res, relu, out32, ds=None, seed=0, subnormal=True):
    """ds = (cin2, H2, W2, stride2): the folded downsample as second A source.  Returns (device result, float64 ref, bound)."""
    rng = np.random.default_rng(seed)
    cp = -(-cin // 8) * 8
    x = np.maximum(rng.standard_normal((B, H, W, cin)), 0) * 1.3
    if subnormal:   # ~4 % of the activations in fp16's subnormal range (the open question of DESIGN.md, settled below)
        x = np.where(rng.random(x.shape) < 0.04, rng.integers(1, 1024, x.shape) * 2.0 ** -24, x)
    x = f16(x)
    w = rng.standard_normal((cout, cin, k, k)) * (2.0 / (cin * k * k)) ** 0.5
    ws = [w]
    if ds:
        cin2, H2, W2, s2 = ds
        x2 = f16(np.maximum(rng.standard_normal((B, H2, W2, cin2)), 0))
        w2 = rng.standard_normal((cout, cin2, 1, 1)) * (1.0 / cin2) ** 0.5
        ws.append(w2)
    sc = (rng.random(cout) + 0.5).astype(np.float32)
    sh = (rng.standard_normal(cout) * 0.1).astype(np.float32)
    if subnormal:   # some folded weights land on fp16 subnormals too
        ws[0] = np.where(rng.random(ws[0].shape) < 0.04, rng.integers(1, 1024, ws[0].shape) * 2.0 ** -24 / sc[:, None, None, None], ws[0])
    wf = [f16(wi.astype(np.float32).astype(np.float64) * sc.astype(np.float64)[:, None, None, None]) for wi in ws]
    nchw = lambda a: np.ascontiguousarray(a.transpose(0, 3, 1, 2))
    acc = _conv64(nchw(x), wf[0], stride, pad)
    sab = _conv64(np.abs(nchw(x)), np.abs(wf[0]), stride, pad)
    if ds:
        x2s = nchw(x2)[:, :, ::s2, ::s2][:, :, :acc.shape[2], :acc.shape[3]]
        acc = acc + _conv64(np.ascontiguousarray(x2s), wf[1], 1, 0)
        sab = sab + _conv64(np.abs(np.ascontiguousarray(x2s)), np.abs(wf[1]), 1, 0)
    ref = acc + sh.astype(np.float64)[None, :, None, None]
    r = None
    if res:
        r = f16(rng.standard_normal(ref.shape))
        ref = ref + r
    if relu:
        ref = np.maximum(ref, 0)
    K = (cin * k * k) + (ds[0] if ds else 0)
    bound = (K / 16 + 4) * 2.0 ** -24 * sab
    xd = torch.zeros(B, H, W, cp, dtype=torch.float16)
    xd[..., :cin] = torch.from_numpy(x)
    kw = {}
    if ds:
        kw = dict(x2=torch.from_numpy(x2).half().to(DEV), w2_oihw=ws[1].astype(np.float32), stride2=s2)
    y = eng.conv2d_f16(xd.to(DEV), ws[0].astype(np.float32), sc, sh, stride, pad,
                       residual=None if r is None else torch.from_numpy(nchw_to_nhwc(r)).half().to(DEV), relu=relu, out_f32=out32, **kw)
    y = y.cpu().double().numpy().transpose(0, 3, 1, 2)
    return y, ref, bound


def _check(y, ref, bound, out32):
    if out32:
        lim = bound + np.abs(ref) * 2.0 ** -23
        err = np.abs(y - ref)
    else:
        r16 = f16(ref)
        ulp = np.spacing(np.abs(r16).astype(np.float16)).astype(np.float64)
        lim = ulp + bound
        err = np.abs(y - r16)
    bad = err > lim
    assert not bad.any(), (int(bad.sum()), float((err / lim).max()), float(err.max()))
    return float((err / np.maximum(lim, 1e-30)).max())


# ---- seeded ragged cases with small-integer operands (tests/test_gpu_fp16_shapes.py, tests/test_fp16_cases_host.py) ---------
# Products are fp16 x fp16 and the device accumulates in fp32: with operands that are small multiples of 0.5 every partial sum, in
# any order, is exact, so the device must equal the float64 reference bit for bit - no tolerance.
CINS = (1, 3, 5, 8, 12, 20, 24, 40, 64, 72, 136, 256)
COUTS = (4, 12, 60, 64, 68, 100, 124, 128, 132, 192, 260, 320)
CINS_2SRC = (32, 64, 96, 128, 256)
X_MAX, W_MAX, SCALES, SHIFT_MAX = 3, 4, (0.5, 1.0, 2.0), 8.0
MAC_BUDGET = 3e8          # multiply-adds of one case's float64 CPU reference; H and W shrink until a case fits


def conv_out(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def case_id(c):
    s = 'B%d_%dx%d_c%d_%d_k%d_s%d_p%d' % (c['B'], c['H'], c['W'], c['cin'], c['cout'], c['k'], c['stride'], c['pad'])
    s += ('_res' if c['res'] else '') + ('_relu' if c['relu'] else '') + ('_f32' if c['out32'] else '')
    return s + ('_ds%d_%dx%d_s%d' % c['ds'] if c['ds'] else '')


def shape_cases(n=72, seed=20240607):
    """n seeded layer shapes as dicts (B, H, W, cin, cout, k, stride, pad, res, relu, out32, ds, seed); every fourth one is a
    two-source case, ds = (cin2, H2, W2, stride2).  Some single-source cases have H or W below k (with the padding that needs),
    the first two two-source cases have the x2 image larger / smaller in bytes than the x image."""
    rng = np.random.default_rng(seed)
    pick = lambda seq: seq[int(rng.integers(len(seq)))]
    cases = []
    for i in range(n):
        B = int(rng.integers(1, 8))
        H, W = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        cout = pick(COUTS)
        res, relu = bool(rng.integers(2)), bool(rng.integers(2))
        if i % 4 == 3:
            cin, cin2, s2 = pick(CINS_2SRC), pick(CINS_2SRC), int(rng.integers(1, 3))
            if i == 3:
                cin, cin2, s2 = 32, 128, 2             # the x2 image is the larger one
            if i == 7:
                cin, cin2, s2 = 256, 32, 1             # ... and the smaller one
            while B * H * W * cout * (cin + cin2) > MAC_BUDGET:
                H, W = max(1, H // 2), max(1, W // 2)
            extra = int(rng.integers(2))               # x2 exactly as large as the last tap needs, or one row / column more
            ds = (cin2, (H - 1) * s2 + 1 + extra, (W - 1) * s2 + 1 + extra, s2)
            cases.append(dict(B=B, H=H, W=W, cin=cin, cout=cout, k=1, stride=1, pad=0, res=res, relu=relu, out32=False, ds=ds))
        else:
            cin, k, stride = pick(CINS), pick((1, 3, 5, 7)), int(rng.integers(1, 4))
            pad = int(rng.integers(0, k))
            if i % 8 == 5 and k > 1:                   # an image narrower or lower than the filter
                if rng.integers(2):
                    H = int(rng.integers(1, k))
                else:
                    W = int(rng.integers(1, k))
            pad0 = pad
            while True:
                pad = max(pad0, -(-(k - min(H, W)) // 2))      # enough padding for one output pixel
                if B * conv_out(H, k, stride, pad) * conv_out(W, k, stride, pad) * cout * cin * k * k <= MAC_BUDGET:
                    break
                H, W = (max(1, H // 2), W) if H >= W else (H, max(1, W // 2))
            cases.append(dict(B=B, H=H, W=W, cin=cin, cout=cout, k=k, stride=stride, pad=pad, res=res, relu=relu,
                              out32=bool(rng.integers(2)), ds=None))
        cases[-1]['seed'] = seed + 1 + i
    return cases


def integer_operands(c):
    """The integer operands of a case as float64 arrays: x (B,H,W,cin) NHWC, w OIHW, scale, shift, res (B,OH,OW,cout) or None,
    x2 (B,H2,W2,cin2) and w2 (cout,cin2,1,1) or None."""
    rng = np.random.default_rng(c['seed'])
    ints = lambda lo, hi, shape: rng.integers(lo, hi + 1, shape).astype(np.float64)
    OH, OW = conv_out(c['H'], c['k'], c['stride'], c['pad']), conv_out(c['W'], c['k'], c['stride'], c['pad'])
    o = dict(x=ints(-X_MAX, X_MAX, (c['B'], c['H'], c['W'], c['cin'])), w=ints(-W_MAX, W_MAX, (c['cout'], c['cin'], c['k'], c['k'])),
             scale=np.asarray(SCALES)[rng.integers(0, len(SCALES), c['cout'])], shift=ints(-2 * SHIFT_MAX, 2 * SHIFT_MAX, c['cout']) * 0.5,
             res=ints(-X_MAX, X_MAX, (c['B'], OH, OW, c['cout'])) if c['res'] else None, x2=None, w2=None)
    if c['ds']:
        cin2, H2, W2, _ = c['ds']
        o['x2'], o['w2'] = ints(-X_MAX, X_MAX, (c['B'], H2, W2, cin2)), ints(-W_MAX, W_MAX, (c['cout'], cin2, 1, 1))
    return o


def layer_reference(o, stride, pad, relu, stride2=1):
    """float64 NHWC reference of one fused layer from operands shaped as integer_operands returns them: the weights are folded
    as the library folds them, fp16_rne(w * scale) from the float64 product, then conv + shift (+ res), ReLU.  No rounding of
    the result: the caller rounds it to fp16 where the device stores fp16."""
    nchw = lambda a: np.ascontiguousarray(a.transpose(0, 3, 1, 2))
    s = o['scale'][:, None, None, None]
    with torch.inference_mode():
        ref = conv64(nchw(o['x']), f16(o['w'] * s), stride, pad)
        if o.get('x2') is not None:
            x2 = nchw(o['x2'])[:, :, ::stride2, ::stride2][:, :, :ref.shape[2], :ref.shape[3]]
            ref = ref + conv64(np.ascontiguousarray(x2), f16(o['w2'] * s), 1, 0)
    ref = nchw_to_nhwc(ref) + o['shift']
    if o.get('res') is not None:
        ref = ref + o['res']
    return np.maximum(ref, 0.0) if relu else ref


def exactness_bound(c, o):
    """max over the outputs of sum |x| |w s| + |shift| + |res| is at most this: K max|x| max|w s| + max|shift| + max|res|."""
    K = c['cin'] * c['k'] ** 2 + (c['ds'][0] if c['ds'] else 0)
    xm = max(np.abs(o['x']).max(), np.abs(o['x2']).max() if o['x2'] is not None else 0.0)
    wm = max(np.abs(o['w'] * o['scale'][:, None, None, None]).max(),
             np.abs(o['w2'] * o['scale'][:, None, None, None]).max() if o['w2'] is not None else 0.0)
    return K * xm * wm + np.abs(o['shift']).max() + (np.abs(o['res']).max() if o['res'] is not None else 0.0)


def run_case(eng, c, o, dev=DEV):
    """One case on the device -> the result as a numpy array (B,OH,OW,cout), float16 or float32 as stored."""
    h = lambda a: None if a is None else torch.from_numpy(a).half().to(dev)
    cp = c['cin'] if c['ds'] else -(-c['cin'] // 8) * 8
    x = torch.zeros(*o['x'].shape[:3], cp, dtype=torch.float16)
    x[..., :c['cin']] = torch.from_numpy(o['x'])
    kw = dict(x2=h(o['x2']), w2_oihw=o['w2'].astype(np.float32), stride2=c['ds'][3]) if c['ds'] else {}
    y = eng.conv2d_f16(x.to(dev), o['w'].astype(np.float32), o['scale'].astype(np.float32), o['shift'].astype(np.float32),
                       c['stride'], c['pad'], residual=h(o['res']), relu=c['relu'], out_f32=c['out32'], **kw)
    return y.cpu().numpy()


def shape_ok(c, ldx=None):
    """conv_f16_shape_ok (conv_f16.hip) restated for a case as specmi_conv2d_f16 lays it out: ldx = cin rounded up to 8 (cin
    itself with two sources), ldo = cout, Npad = cout rounded up to 64, Kp = K rounded up to 32."""
    cin, cout, k, stride, pad = c['cin'], c['cout'], c['k'], c['stride'], c['pad']
    ldx = ldx or (cin if c['ds'] else -(-cin // 8) * 8)
    npad = -(-cout // 64) * 64
    OH, OW = conv_out(c['H'], k, stride, pad), conv_out(c['W'], k, stride, pad)
    if c['B'] <= 0 or cin <= 0 or ldx % 8 or ldx < cin or cout % 4 or k < 1 or stride < 1 or pad < 0 or OH < 1 or OW < 1:
        return False
    if c['ds']:
        cin2, H2, W2, s2 = c['ds']
        if (k != 1 or stride != 1 or pad != 0 or cin % 32 or cin2 % 32 or s2 < 1 or (OH - 1) * s2 >= H2 or (OW - 1) * s2 >= W2
                or c['out32']):
            return False
        kp = cin + cin2
    else:
        kp = -(-(k * k * ldx) // 32) * 32
    img = max(c['H'] * c['W'] * ldx * 2, c['ds'][1] * c['ds'][2] * c['ds'][0] * 2 if c['ds'] else 0)
    return kp * npad * 2 < 2 ** 31 and img < 2 ** 31


def instance(c):
    """The conv_f16_kernel instance launch_conv_f16 picks: (wide tile, two sources, fp32 out)."""
    return (-(-c['cout'] // 64) * 64) % 128 == 0, c['ds'] is not None, c['out32']


INSTANCE_NAMES = {(True, False, False): 'conv_f16<128x128>', (False, False, False): 'conv_f16<128x64>',
                  (True, True, False): 'conv_f16<128x128,2src>', (False, True, False): 'conv_f16<128x64,2src>',
                  (True, False, True): 'conv_f16<128x128,f32 out>', (False, False, True): 'conv_f16<128x64,f32 out>'}


def tie_case():
    """Sums that land exactly on fp16 store ties: x (1,1,4,8) with channel sums 2049, 2051, 4098, 4102 under w = 1, scale = 1,
    shift = 0, and the fp16 values round-to-nearest-even makes of them."""
    x = np.zeros((1, 1, 4, 8))
    x[0, 0, :, 0] = (2048, 2048, 2048, 2048)
    x[0, 0, :, 1] = (1, 3, 2048, 2048)
    x[0, 0, :, 2] = (0, 0, 2, 6)
    return x, np.array([2049.0, 2051.0, 4098.0, 4102.0]), np.array([2048.0, 2052.0, 4096.0, 4104.0])


# ---- the batch split of launch_conv_f16 beyond 2 GiB (tests/test_gpu_fp16_shapes.py builds the operands on the device) -------
# side: which tensor crosses 2 GiB.  The x2 case is past 4 GiB as well: between 2 and 4 GiB a launch that wrongly took the whole
# batch would still address all but one pixel correctly through unsigned wrap-around, and the case would not tell.
SPLIT_CASES = [
    dict(side='x', B=132, H=64, W=64, cin=2048, cout=64, k=1, stride=1, pad=0, res=True, relu=True, out32=False, ds=None),
    dict(side='x2', B=260, H=32, W=32, cin=32, cout=64, k=1, stride=1, pad=0, res=False, relu=False, out32=False, ds=(2048, 64, 64, 2)),
    dict(side='out', B=176, H=224, W=224, cin=16, cout=64, k=3, stride=1, pad=1, res=False, relu=True, out32=True, ds=None),
]


def split_images_per_launch(c):
    """launch_conv_f16's rule: whole images per launch so that neither A source of a launch reaches 2 GiB."""
    ldx = c['cin'] if c['ds'] else -(-c['cin'] // 8) * 8
    img = max(c['H'] * c['W'] * ldx * 2, c['ds'][1] * c['ds'][2] * c['ds'][0] * 2 if c['ds'] else 0)
    return (2 ** 31 - 1) // img


def split_probe_images(c):
    """The images compared with the CPU reference: first, last, both sides of every launch boundary and of every 2 GiB line of
    the output."""
    per, B = split_images_per_launch(c), c['B']
    idx = {0, B - 1}
    for b in range(per, B, per):
        idx |= {b - 1, b}
    oimg = conv_out(c['H'], c['k'], c['stride'], c['pad']) * conv_out(c['W'], c['k'], c['stride'], c['pad']) * c['cout'] * (4 if c['out32'] else 2)
    for line in range(2 ** 31, B * oimg, 2 ** 31):
        b = line // oimg
        idx |= {max(b - 1, 0), b, min(b + 1, B - 1)}
    return sorted(idx)


def split_operands(c, B, device, seed=5):
    """Integer operands of a split case as torch tensors on ``device``: x, x2, res fp16 NHWC (or None); w, w2, scale, shift as
    float64 numpy arrays.  Values as in integer_operands."""
    g = torch.Generator(device=device).manual_seed(seed)
    ints = lambda *shape: torch.randint(-X_MAX, X_MAX + 1, shape, generator=g, device=device, dtype=torch.int8).half()
    OH, OW = conv_out(c['H'], c['k'], c['stride'], c['pad']), conv_out(c['W'], c['k'], c['stride'], c['pad'])
    cp = c['cin'] if c['ds'] else -(-c['cin'] // 8) * 8
    x = ints(B, c['H'], c['W'], cp)
    x[..., c['cin']:] = 0
    rng = np.random.default_rng(seed)
    o = dict(x=x, x2=None, w2=None, res=ints(B, OH, OW, c['cout']) if c['res'] else None,
             w=rng.integers(-W_MAX, W_MAX + 1, (c['cout'], c['cin'], c['k'], c['k'])).astype(np.float64),
             scale=np.asarray(SCALES)[rng.integers(0, len(SCALES), c['cout'])],
             shift=rng.integers(-2 * SHIFT_MAX, 2 * SHIFT_MAX + 1, c['cout']) * 0.5)
    if c['ds']:
        cin2, H2, W2, _ = c['ds']
        o['x2'] = ints(B, H2, W2, cin2)
        o['w2'] = rng.integers(-W_MAX, W_MAX + 1, (c['cout'], cin2, 1, 1)).astype(np.float64)
    return o


def split_reference(c, o, images):
    """float64 NHWC reference of the listed images of a split case (operands from split_operands)."""
    sel = lambda a: None if a is None else a[images].cpu().double().numpy()
    oo = dict(o, x=sel(o['x'])[..., :c['cin']], x2=sel(o['x2']), res=sel(o['res']))
    return layer_reference(oo, c['stride'], c['pad'], c['relu'], c['ds'][3] if c['ds'] else 1)
