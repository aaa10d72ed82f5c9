"""Test reference: the CNN restated in torch on the CPU with batch-moment BN, so that autograd supplies exact gradients: the
counterpart of tests/rnn_ref.py.

A restatement of oracle/nn_oracle.py (same_padding, conv1d_same as explicit tap sums, bn_apply's association order, residual_layer,
cnn_forward) with bn_mode "batch": moments over axes (0, 1) of each site's own output, biased variance, epsilon float32(1e-5).
tests/test_cnn_train_cpu.py pins its float64 forward to the oracle at 1e-12.  Run in float32 it is the yardstick of the gradient tests:
one more float32 realisation of the same formulas, in torch's accumulation order.  `draw` makes further realisations of the same
formulas for the ensemble that sets the tests' FACTOR (tools/cnn_grad_accuracy.py): every convolution's input and output channels
in a permuted order (un-permuted afterwards) and the batch in another order.

`masks`.  A ReLU whose pre-activation is within rounding of 0 flips between float32 realisations and moves every upstream gradient by
a discrete amount, so gradients of two realisations cannot be held to each other under a bar of a few rounding errors.  With `masks`
({relu name: bool [B, T, C]}) every ReLU is `y * mask` instead: the function is smooth, and it equals the network wherever the masks
are the signs of the pre-activations.  The GPU tests take the masks from the implementation under test (its ReLU outputs > 0),
check that they differ from the float64 signs only where the float64 pre-activation is within rounding of 0, and then compare
gradients under the same masks.  ReLU names: the stem's site, <block>/branch2/conv2a, <block>/branch2/conv2b, <block>/out."""
import numpy as np
import torch

BN_EPS = float(np.float32(1e-5))


def same_padding(width, k, stride):
    out = -(-width // stride)
    pad_total = max((out - 1) * stride + k - width, 0)
    left = pad_total // 2
    return out, left, pad_total - left


def conv1d_same(x, w, stride, rng=None):
    """x [B, W, Cin], w [k, Cin, Cout] -> [B, ceil(W / stride), Cout]; rng: permute the channels of both sides for this product."""
    B, W, Cin = x.shape
    k, _, Cout = w.shape
    out, left, right = same_padding(W, k, stride)
    xp = torch.nn.functional.pad(x, (0, 0, left, right))
    if rng is not None:
        pi, po = torch.from_numpy(rng.permutation(Cin)), torch.from_numpy(rng.permutation(Cout))
        xp, w = xp[:, :, pi], w[:, pi][:, :, po]
    y = None
    for tap in range(k):
        term = xp[:, tap:tap + (out - 1) * stride + 1:stride] @ w[tap]
        y = term if y is None else y + term
    if rng is not None:
        y = y[:, :, torch.argsort(po)]
    return y


def bn_batch(x, scale, offset):
    mean = x.mean(dim=(0, 1))
    var = ((x - mean) ** 2).mean(dim=(0, 1))
    inv = (1.0 / torch.sqrt(var + BN_EPS)) * scale
    return x * inv + (offset - mean * inv), mean, var


def cnn_forward(signal, spec_obj, w, rng=None, masks=None, pre=None):
    """signal tensor [B, L]; w: {canonical name: tensor} -> (features [B, T, C], {site: (mean, var)}).  masks: see the module
    docstring; pre: a dict that receives every ReLU's detached pre-activation."""
    moments = {}

    def act(y, name):
        if pre is not None:
            pre[name] = y.detach()
        return torch.relu(y) if masks is None else y * masks[name].to(y.dtype)

    def site(x, name, stride, bn, relu):
        f = w[name + "/weights"]
        y = conv1d_same(x, f.reshape(f.shape[-3], f.shape[-2], f.shape[-1]), stride, rng)
        if bn:
            y, m, v = bn_batch(y, w[name + "_bn/scale"], w[name + "_bn/offset"])
            moments[name] = (m, v)
        return act(y, name) if relu else y

    x = signal[:, :, None]
    if spec_obj.stem:
        x = site(x, spec_obj.STEM_SITE, spec_obj.stem["stride"], True, True)
    for blk in spec_obj.blocks:
        n, s = blk["name"], blk["stride"]
        b1 = site(x, n + "/branch1/conv1", s, blk["i_bn"], False)
        a = site(x, n + "/branch2/conv2a", 1, True, True)
        b = site(a, n + "/branch2/conv2b", s, True, True)
        c = site(b, n + "/branch2/conv2c", 1, True, False)
        x = act(b1 + c, n + "/out")
    return x, moments


def trainable_names(spec_obj):
    """The canonical names of the CNN's trainable tensors: filters, BN scale and offset."""
    rnn = set(n for n, _ in spec_obj._rnn_and_head())
    return [n for n in spec_obj.blob_layout() if n not in rnn and not n.endswith(("_bn/pop_mean", "_bn/pop_var"))]


def leaves(spec_obj, weights, dtype, requires_grad=False):
    canon = spec_obj.canonical_weights(weights)
    return {k: torch.tensor(np.asarray(canon[k]), dtype=dtype, requires_grad=requires_grad) for k in trainable_names(spec_obj)}


def forward(signal, spec_obj, weights, dtype=torch.float64, draw=None):
    """numpy in -> (features, {site: (mean, var)}) as float64 numpy arrays (computed in `dtype`); draw: as in `gradients`."""
    with torch.no_grad():
        x = torch.tensor(np.asarray(signal), dtype=dtype)
        rng = None
        if draw is not None:
            rng = np.random.RandomState(draw)
            order = torch.from_numpy(rng.permutation(x.shape[0]))
            x = x[order]
        fea, mom = cnn_forward(x, spec_obj, leaves(spec_obj, weights, dtype), rng)
        if draw is not None:
            fea = fea[torch.argsort(order)]
    return fea.to(torch.float64).numpy(), {k: (m.to(torch.float64).numpy(), v.to(torch.float64).numpy()) for k, (m, v) in mom.items()}


def gradients(signal, spec_obj, weights, dfeatures, dtype=torch.float64, draw=None, masks=None, pre=None):
    """-> (features, {name: d sum(features * dfeatures) / d name}) as float64 numpy arrays (computed in `dtype`).  draw: an int seed of
    one more realisation (channel orders of every product, batch order).  masks: {relu name: bool numpy [B, T, C]} (module
    docstring); pre: a dict that receives the ReLUs' pre-activations as numpy arrays (not with draw)."""
    w = leaves(spec_obj, weights, dtype, requires_grad=True)
    x = torch.tensor(np.asarray(signal), dtype=dtype)
    g = torch.tensor(np.asarray(dfeatures), dtype=dtype)
    rng = None
    if draw is not None:
        rng = np.random.RandomState(draw)
        order = torch.from_numpy(rng.permutation(x.shape[0]))
        x, g = x[order], g[order]
    m = None
    if masks is not None:
        m = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in masks.items()}
        if draw is not None:
            m = {k: v[order] for k, v in m.items()}
    raw = {} if pre is not None else None
    fea, _ = cnn_forward(x, spec_obj, w, rng, m, raw)
    if pre is not None:
        pre.update((k, v.to(torch.float64).numpy()) for k, v in raw.items())
    (fea * g).sum().backward()
    if draw is not None:
        fea = fea[torch.argsort(order)]
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach().to(torch.float64).numpy() for k, v in w.items()}
    return fea.detach().to(torch.float64).numpy(), grads
