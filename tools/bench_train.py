#!/usr/bin/env python
"""Time forward + backward of the recurrent stack and the FC head at the reference's training shape (batch 300, T 400, C 256:
chiron_rcnn_train.py:192-195) on the HIP path (chiron_rnn_train_forward / _backward) and on the obvious alternative,
torch.nn.LSTM(256, 100, num_layers=3, bidirectional=True) plus the head in torch, on the same GPU.  Full-length rows, so that the
two compute the same thing.  The two are run interleaved in one process and compared by their medians; the result goes to
profiles/train_step.json.  Needs a GPU: there is nothing to time without one."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=300)
    ap.add_argument("-T", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_step.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_train.py needs a GPU")
    torch.cuda.init()
    import chiron_amd as ca
    from chiron_amd import train
    spec = ca.dna_default_spec()
    w = ca.synthetic_weights(spec, seed=7)
    dev = torch.device("cuda", 0)
    B, T, C, H = args.batch, args.T, 256, 100
    rng = np.random.default_rng(1)
    x = torch.from_numpy(np.maximum(rng.normal(size=(B, T, C)), 0).astype(np.float32)).to(dev)
    sl = torch.full((B,), T, dtype=torch.int32, device=dev)
    dl = torch.from_numpy(rng.normal(size=(B, T, 5)).astype(np.float32)).to(dev)
    head = train.RecurrentHead(spec, w)

    def hip_step():
        head.flat.grad = None
        (head(x, sl) * dl).sum().backward()

    result = {"batch": B, "T": T, "C": C, "hidden": H, "layers": 3, "rounds": args.rounds, "device": torch.cuda.get_device_name(0)}
    try:
        lstm = torch.nn.LSTM(C, H, num_layers=3, bidirectional=True, batch_first=True).to(dev)
        fw = torch.nn.Parameter(torch.randn(2, H, device=dev))
        fb = torch.nn.Parameter(torch.randn(H, device=dev))
        wc = torch.nn.Parameter(torch.randn(H, 5, device=dev))
        bc = torch.nn.Parameter(torch.randn(5, device=dev))

        def torch_step():
            for p in list(lstm.parameters()) + [fw, fb, wc, bc]:
                p.grad = None
            out, _ = lstm(x)
            v = (out.reshape(B, T, 2, H) * fw).sum(dim=2) + fb
            ((v @ wc + bc) * dl).sum().backward()

        torch_step()
        torch.cuda.synchronize()
    except Exception as e:   # torch's LSTM does not run on this build: recorded in place of the ratio
        torch_step = None
        result["torch_lstm_error"] = "%s: %s" % (type(e).__name__, str(e)[:300])

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(args.warmup):
        hip_step()
        if torch_step:
            torch_step()
    hip_ms, torch_ms = [], []
    for _ in range(args.rounds):      # interleaved: both see the same machine state
        hip_ms.append(timed(hip_step))
        if torch_step:
            torch_ms.append(timed(torch_step))
    result["hip_ms"] = {"median": float(np.median(hip_ms)), "min": float(np.min(hip_ms)), "max": float(np.max(hip_ms))}
    if torch_ms:
        result["torch_lstm_ms"] = {"median": float(np.median(torch_ms)), "min": float(np.min(torch_ms)), "max": float(np.max(torch_ms))}
        result["ratio_torch_over_hip"] = result["torch_lstm_ms"]["median"] / result["hip_ms"]["median"]
    tape, ws = train.train_sizes(spec, B, T)
    result["tape_bytes"], result["workspace_bytes"] = tape, ws
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
