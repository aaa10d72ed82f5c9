#!/usr/bin/env python
"""Time the CNN training seam and the whole training step at the reference's training shape (batch 300, segment 400, DNA_default:
chiron_rcnn_train.py:192-195), in one process, in interleaved rounds, with torch events:

1. the CNN forward + backward alone through chiron_cnn_train_forward / _backward;
2. the same CNN in torch on the same GPU (F.conv1d + batch-moment BN + autograd, fp32): the baseline, in two forms: BN composed
   from mean / square / rsqrt / multiply-add in TF's association order (every step a tensor of its own under autograd), and BN as
   F.batch_norm(training=True), what a torch user would call (fused forward and backward);
3. the full step through train.Network (CNN, recurrent stack, head, chiron_ctc_loss and its gradient, full backward), next to the
   recurrent seam alone (RecurrentHead on fixed features), so that the CNN's share of a step is visible.

The HIP leg is timed through the Python wrappers as a caller pays for it: each call allocates its tape and workspace (torch's caching
allocator), zeroes the moments vector and checks every pointer's residency.  Medians and ranges go to profiles/train_step_full.json.  Needs a GPU: there is nothing to time without one."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CNN_FLOP_FLOOR_MS = 4.8   # 0.75 TFLOP a step (0.25 forward, twice that backward) at the 157 TFLOP/s fp32-MFMA peak: derived, not measured


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=300)
    ap.add_argument("--segment", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_step_full.json"))
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_full.py needs a GPU")
    torch.cuda.init()
    import chiron_amd as ca
    from chiron_amd import train
    spec = ca.dna_default_spec()
    w = ca.synthetic_weights(spec, seed=7)
    dev = torch.device("cuda", 0)
    B, L = args.batch, args.segment
    T, C = spec.output_len(L), 256
    rng = np.random.default_rng(1)
    x = torch.from_numpy(ca.synthetic_signal(B, L, seed=5)).to(dev)
    dfea = torch.from_numpy(rng.normal(size=(B, T, C)).astype(np.float32)).to(dev)
    sl = torch.full((B,), T, dtype=torch.int32, device=dev)
    ll = np.full(B, 40, dtype=np.int32)
    lab = torch.from_numpy(rng.integers(0, 4, size=(B, 40)).astype(np.int32)).to(dev)
    ll_d = torch.from_numpy(ll).to(dev)
    n_cnn = train.cnn_params_range(spec)[1]
    p_cnn = torch.from_numpy(spec.pack(w)[:n_cnn].copy()).to(dev)

    def hip_cnn():
        fea, _, tape, ws = train.cnn_forward(spec, p_cnn, x)
        train.cnn_backward(spec, p_cnn, x, dfea, tape, ws)

    # the same CNN in torch: [B, C, T] layout, filters [co, ci, k], TF SAME padding by hand, moments over (0, 2)
    canon = spec.canonical_weights(w)
    tw = {k: torch.nn.Parameter(torch.from_numpy(np.asarray(v, dtype=np.float32)).to(dev)) for k, v in canon.items() if "res_layer" in k}

    def t_site(h, name, k, stride, bn, relu, fused=False):
        f = tw[name + "/weights"]
        f = f.reshape(f.shape[-3], f.shape[-2], f.shape[-1]).permute(2, 1, 0)
        W = h.shape[2]
        out = -(-W // stride)
        tot = max((out - 1) * stride + k - W, 0)
        y = F.conv1d(F.pad(h, (tot // 2, tot - tot // 2)), f, stride=stride)
        if bn and fused:
            y = F.batch_norm(y, None, None, tw[name + "_bn/scale"], tw[name + "_bn/offset"], training=True, eps=1e-5)
        elif bn:
            mean = y.mean(dim=(0, 2), keepdim=True)
            var = ((y - mean) ** 2).mean(dim=(0, 2), keepdim=True)
            inv = torch.rsqrt(var + 1e-5) * tw[name + "_bn/scale"][None, :, None]
            y = y * inv + (tw[name + "_bn/offset"][None, :, None] - mean * inv)
        return torch.relu(y) if relu else y

    dfea_t = dfea.permute(0, 2, 1).contiguous()

    def torch_cnn(fused=False):
        for p in tw.values():
            p.grad = None
        h = x[:, None, :]
        for b in spec.blocks:
            n, s = b["name"], b["stride"]
            b1 = t_site(h, n + "/branch1/conv1", 1, s, b["i_bn"], False, fused)
            a = t_site(h, n + "/branch2/conv2a", 1, 1, True, True, fused)
            a = t_site(a, n + "/branch2/conv2b", b["k"], s, True, True, fused)
            h = torch.relu(b1 + t_site(a, n + "/branch2/conv2c", 1, 1, True, False, fused))
        (h * dfea_t).sum().backward()

    def torch_cnn_fused():
        torch_cnn(True)

    net = train.Network(spec, w)
    net.eval()   # the statistics stay put: every round times the same weights

    def full_step():
        net.flat.grad = None
        train.batch_loss(net(x, sl), sl, lab, ll_d).backward()

    head = train.RecurrentHead(spec, w)
    fea0 = train.cnn_forward(spec, p_cnn, x)[0]
    dl = torch.from_numpy(rng.normal(size=(B, T, 5)).astype(np.float32)).to(dev)

    def rnn_seam():
        head.flat.grad = None
        (head(fea0, sl) * dl).sum().backward()

    legs = [("hip_cnn_ms", hip_cnn), ("torch_cnn_ms", torch_cnn), ("torch_cnn_fused_bn_ms", torch_cnn_fused), ("full_step_ms", full_step), ("rnn_seam_ms", rnn_seam)]

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    for _ in range(args.warmup):
        for _, fn in legs:
            fn()
    ms = {name: [] for name, _ in legs}
    for _ in range(args.rounds):      # interleaved: every leg sees the same machine state
        for name, fn in legs:
            ms[name].append(timed(fn))
    result = {"batch": B, "segment": L, "T": T, "model": "DNA_default", "rounds": args.rounds, "device": torch.cuda.get_device_name(0)}
    for name, v in ms.items():
        result[name] = {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
    result["ratio_torch_over_hip_cnn"] = result["torch_cnn_ms"]["median"] / result["hip_cnn_ms"]["median"]
    result["ratio_torch_fused_bn_over_hip_cnn"] = result["torch_cnn_fused_bn_ms"]["median"] / result["hip_cnn_ms"]["median"]
    result["cnn_share_of_step"] = result["hip_cnn_ms"]["median"] / result["full_step_ms"]["median"]
    result["cnn_flop_floor_ms"] = CNN_FLOP_FLOOR_MS
    result["cnn_fraction_of_flop_floor"] = CNN_FLOP_FLOOR_MS / result["hip_cnn_ms"]["median"]
    tape, ws = train.cnn_train_sizes(spec, B, L)
    result["cnn_tape_bytes"], result["cnn_workspace_bytes"] = tape, ws
    rt, rw = train.train_sizes(spec, B, T)
    result["rnn_tape_bytes"], result["rnn_workspace_bytes"] = rt, rw
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
