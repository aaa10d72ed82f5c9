"""Test reference: the recurrent stack and the FC head restated in torch on the CPU, so that autograd supplies exact gradients.

A restatement of oracle/nn_oracle.py (lstm_direction, the stack / multi wiring of rnn_forward, fc_head): gate order i, j, f, o,
forget bias +1.0, frames t >= seq_len[b] emit 0 and carry the state, the backward direction runs over the first seq_len[b] frames
reversed.  tests/test_rnn_ref_cpu.py pins its float64 forward to the oracle at 1e-12.  Run in float32 it is the yardstick of the
gradient tests: one more float32 realisation of the same formulas, in torch's accumulation order."""
import numpy as np
import torch

FORGET_BIAS = 1.0


def lstm_direction(x, seq_len, kernel, bias, reverse):
    """x [B, T, K], seq_len int64 [B] -> [B, T, H]."""
    B, T, _ = x.shape
    H = kernel.shape[1] // 4
    h = x.new_zeros((B, H))
    c = x.new_zeros((B, H))
    rows = torch.arange(B)
    steps = int(seq_len.max()) if B else 0
    emitted = []
    for step in range(steps):
        active = step < seq_len
        t_idx = torch.where(active, seq_len - 1 - step, torch.zeros_like(seq_len)) if reverse else torch.full_like(seq_len, step)
        z = torch.cat([x[rows, t_idx], h], dim=1) @ kernel + bias
        i, j, f, o = z[:, :H], z[:, H:2 * H], z[:, 2 * H:3 * H], z[:, 3 * H:]
        c_new = torch.sigmoid(f + FORGET_BIAS) * c + torch.sigmoid(i) * torch.tanh(j)
        h_new = torch.sigmoid(o) * torch.tanh(c_new)
        m = active[:, None]
        c = torch.where(m, c_new, c)
        h = torch.where(m, h_new, h)
        emitted.append(torch.where(m, h_new, torch.zeros_like(h_new)))
    if steps == 0:
        return x.new_zeros((B, T, H))
    by_step = torch.stack(emitted, dim=1)                      # [B, steps, H], 0 past the row's end
    frames = torch.arange(T)[None, :].expand(B, T)
    live = frames < seq_len[:, None]
    src = torch.where(live, seq_len[:, None] - 1 - frames, torch.zeros_like(frames)) if reverse else frames.clamp(max=steps - 1)
    out = torch.gather(by_step, 1, src[:, :, None].expand(B, T, H))
    return torch.where(live[:, :, None], out, torch.zeros_like(out))


def rnn_forward(fea, seq_len, spec, weights):
    """spec: ModelSpec.to_dict(); weights: {name: tensor}.  Layer by layer as nn_oracle.rnn_layer_forward (equal to rnn_forward)."""
    r = spec["rnn"]
    H = r["hidden"]
    x = fea
    for layer in range(r["layers"]):
        outs = []
        for di, (d, rev) in enumerate((("fw", False), ("bw", True))):
            if r["kind"] == "stack":
                p = "BDLSTM_rnn/cell_%d/bidirectional_rnn/%s/lstm_cell/" % (layer, d)
                xin = x
            else:
                p = "BDGRU_rnn/%s/multi_rnn_cell/cell_%d/lstm_cell/" % (d, layer)
                xin = x if layer == 0 else x[:, :, di * H:(di + 1) * H]
            outs.append(lstm_direction(xin, seq_len, weights[p + "kernel"], weights[p + "bias"], rev))
        x = torch.cat(outs, dim=2)
    return x


def fc_head(lasth, weights):
    B, T, H2 = lasth.shape
    H = H2 // 2
    v = (lasth.reshape(B, T, 2, H) * weights["rnn_fnn_layer/weights"]).sum(dim=2) + weights["rnn_fnn_layer/bias"]
    return v @ weights["rnn_fnn_layer/weights_class"] + weights["rnn_fnn_layer/bias_class"]


def trainable_names(spec_obj):
    return [name for name, _ in spec_obj._rnn_and_head()]


def forward(fea, seq_len, spec_obj, weights, dtype=torch.float64, requires_grad=False):
    """numpy in -> (logits tensor, {name: leaf tensor}, features leaf tensor)."""
    names = trainable_names(spec_obj)
    w = {k: torch.tensor(np.asarray(weights[k]), dtype=dtype, requires_grad=requires_grad) for k in names}
    x = torch.tensor(np.asarray(fea), dtype=dtype, requires_grad=requires_grad)
    sl = torch.tensor(np.asarray(seq_len), dtype=torch.int64)
    return fc_head(rnn_forward(x, sl, spec_obj.to_dict(), w), w), w, x


def gradients(fea, seq_len, spec_obj, weights, dlogits, dtype=torch.float64):
    """-> (logits, {name: d sum(logits * dlogits) / d name}, dfeatures) as float64 numpy arrays (computed in `dtype`)."""
    logits, w, x = forward(fea, seq_len, spec_obj, weights, dtype, requires_grad=True)
    (logits * torch.tensor(np.asarray(dlogits), dtype=dtype)).sum().backward()
    g = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach().to(torch.float64).numpy() for k, v in w.items()}
    return logits.detach().to(torch.float64).numpy(), g, x.grad.detach().to(torch.float64).numpy()
