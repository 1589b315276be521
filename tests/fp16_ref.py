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


def _layout(depth):
    basic = depth in (18, 34)
    nblocks = {18: (2, 2, 2, 2), 34: (3, 4, 6, 3), 50: (3, 4, 6, 3), 101: (3, 4, 23, 3), 152: (3, 8, 36, 3)}[depth]
    return basic, nblocks


def trunk(sd, images, prefix='backbone.', depth=50):
    """images (B,3,H,W) float -> layer4 features (B,C,h,w) float64 under the fp16 contract."""
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
