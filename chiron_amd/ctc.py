"""CTC loss, its gradient, and the normalized edit distance: the scoring half of the reference's training loop,
chiron_model.loss (chiron/chiron_model.py:50-75: tf.nn.ctc_loss, ctc_merge_repeated=True,
ignore_longer_outputs_than_inputs=True) and chiron_model.prediction (:101-132: tf.edit_distance(..., normalize=True)).

The loss and gradient run on the GPU (chiron_ctc_loss, csrc/ctc_loss.hip); there is no CPU fallback.  The edit-distance
helpers here are host code for summaries and checks; on the engine's own decode the distance runs on the GPU
(Engine.score).

Conventions (include/chiron_amd.h): classes A,C,G,T = 0..3, blank = 4; per row, loss 0 and status 1 when label_len > seq_len
(skipped), loss +inf and status 2 when the labels do not fit once every repeat has its blank (infeasible), zero gradient for
both and for every frame t >= seq_len.
"""
import ctypes as C

import numpy as np

from . import _lib

STATUS_SCORED, STATUS_SKIPPED, STATUS_INFEASIBLE = 0, 1, 2


def _torch():
    import torch
    return torch


def _is_torch_cuda(x):
    return hasattr(x, "data_ptr") and hasattr(x, "is_cuda") and x.is_cuda


def row_status(seq_len, labels, label_len):
    """The per-row status the kernels give (host restatement): 0 scored, 1 skipped, 2 infeasible."""
    labels = np.asarray(labels)
    out = np.zeros(len(label_len), dtype=np.int32)
    for b, (t, n) in enumerate(zip(np.asarray(seq_len), np.asarray(label_len))):
        lab = labels[b, :n]
        rep = int(np.count_nonzero(lab[1:] == lab[:-1])) if n > 1 else 0
        out[b] = STATUS_SKIPPED if n > t else (STATUS_INFEASIBLE if n + rep > t else STATUS_SCORED)
    return out


def _launch(logits, seq_len, labels, label_len, want_grad, check=True):
    """torch CUDA tensors in (float32 [B,T,5], int32 [B], int32 [B,Lmax], int32 [B]) -> (loss [B], grad [B,T,5] or None), enqueued on
    torch.cuda.current_stream().  check=False: the caller vouches for seq_len / labels / label_len (CHIRON_CTC_TRUSTED): no
    read-back, no synchronisation."""
    torch = _torch()
    if logits.dim() != 3 or logits.shape[2] != _lib.CLASSES:
        raise ValueError("logits must be [batch, T, %d]" % _lib.CLASSES)
    if labels.dim() != 2 or labels.shape[0] != logits.shape[0] or seq_len.shape[0] != logits.shape[0] or label_len.shape[0] != logits.shape[0]:
        raise ValueError("seq_len / label_len [batch] and labels [batch, max_label_len] must match logits' batch")
    dev = logits.device
    logits = logits.detach().to(torch.float32).contiguous()
    seq_len = seq_len.to(device=dev, dtype=torch.int32).contiguous()
    labels = labels.to(device=dev, dtype=torch.int32).contiguous()
    label_len = label_len.to(device=dev, dtype=torch.int32).contiguous()
    B, T, _ = logits.shape
    lmax = labels.shape[1]
    lib = _lib.load()
    flags = (_lib.CTC_WANT_GRAD if want_grad else 0) | (0 if check else _lib.CTC_TRUSTED)
    nbytes = C.c_size_t()
    _lib.check(lib.chiron_ctc_workspace_size(B, T, lmax, flags, C.byref(nbytes)))
    loss = _lib.device_output((B,), torch.float32, dev)
    grad = _lib.device_output((B, T, _lib.CLASSES), torch.float32, dev) if want_grad else None
    ws = _lib.device_bytes(nbytes.value, dev, at_least=4) if want_grad else None
    stream = torch.cuda.current_stream(dev)
    if B > 0:
        _lib.check(lib.chiron_ctc_loss(dev.index if dev.index is not None else torch.cuda.current_device(), logits.data_ptr(),
                                       seq_len.data_ptr(), labels.data_ptr() if labels.numel() else label_len.data_ptr(), label_len.data_ptr(),
                                       B, T, lmax, flags, loss.data_ptr(), grad.data_ptr() if want_grad else None,
                                       ws.data_ptr() if want_grad else None, C.c_void_p(stream.cuda_stream)))
    if ws is not None:
        ws.record_stream(stream)
    return loss, grad


def ctc_loss(logits, seq_len, labels, label_len, want_grad=False, check=True):
    """Per-row CTC loss (and, with want_grad, d loss / d logits) on the GPU.

    numpy arrays are copied to the device and the results come back as numpy arrays; torch CUDA tensors are used in place
    (zero-copy, on torch.cuda.current_stream()) and the results are CUDA tensors.  -> loss [B], or (loss, grad [B, T, 5]).
    check=False skips the argument check (and the stream synchronisation it costs) for inputs the caller has checked."""
    if _is_torch_cuda(logits):
        loss, grad = _launch(logits, seq_len, labels, label_len, want_grad, check)
        return (loss, grad) if want_grad else loss
    torch = _torch()
    dev = torch.device("cuda", torch.cuda.current_device())
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)   # noqa: E731
    labels = np.asarray(labels)
    if labels.ndim == 1:
        labels = labels.reshape(len(label_len), -1)
    loss, grad = _launch(t(logits, np.float32), t(seq_len, np.int32), t(labels, np.int32), t(label_len, np.int32), want_grad, check)
    torch.cuda.current_stream(dev).synchronize()
    return (loss.cpu().numpy(), grad.cpu().numpy()) if want_grad else loss.cpu().numpy()


def _make_ctc_function():
    torch = _torch()

    class CTCLoss(torch.autograd.Function):
        """loss = CTCLoss.apply(logits, seq_len, labels, label_len): per-row CTC loss whose backward is the HIP gradient
        (chiron_ctc_loss with CHIRON_CTC_WANT_GRAD) scaled by the incoming gradient of each row.  Rows with an infinite loss
        (infeasible) have a zero gradient; a caller that sums the losses should mask them out first."""

        @staticmethod
        def forward(ctx, logits, seq_len, labels, label_len):
            loss, grad = _launch(logits, seq_len, labels, label_len, want_grad=logits.requires_grad)
            ctx.save_for_backward(grad if grad is not None else loss.new_zeros(0))
            return loss

        @staticmethod
        def backward(ctx, grad_loss):
            (grad,) = ctx.saved_tensors
            if grad.numel() == 0:
                return None, None, None, None
            return grad * grad_loss.reshape(-1, 1, 1), None, None, None

    return CTCLoss


_CTC_FN = None


def __getattr__(name):
    # CTCLoss is built on first use, so that importing this module needs no torch
    global _CTC_FN
    if name == "CTCLoss":
        if _CTC_FN is None:
            _CTC_FN = _make_ctc_function()
        return _CTC_FN
    raise AttributeError(name)


# ---------------------------------------------------------------------------------------------
# edit distance, host side
# ---------------------------------------------------------------------------------------------
def levenshtein(a, b):
    """Plain Levenshtein distance (unit insert / delete / substitute) of two sequences."""
    a = list(a)
    b = list(b)
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        ai = a[i - 1]
        for j in range(1, len(b) + 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ai != b[j - 1]))
        prev = cur
    return prev[len(b)]


def normalized_edit_distance(hyp, truth):
    """tf.edit_distance(..., normalize=True) for one row: distance / len(truth), as float32; an empty truth gives 0 against an
    empty hypothesis and +inf otherwise (recalled TF behaviour)."""
    d = levenshtein(hyp, truth)
    if len(truth) == 0:
        return np.float32(0.0) if len(hyp) == 0 else np.float32(np.inf)
    return np.float32(d) / np.float32(len(truth))


def sparse_rows(indices, values, batch):
    """SparseTensor (indices [nnz, 2], values [nnz]) -> one list of labels per row."""
    rows = [[] for _ in range(batch)]
    for (r, _), v in zip(np.asarray(indices).reshape(-1, 2), np.asarray(values)):
        rows[int(r)].append(int(v))
    return rows


def edit_distance(hyp_rows, labels, label_len):
    """Normalized edit distance of every row: hyp_rows a list of label sequences, labels [B, Lmax] padded, label_len [B]."""
    labels = np.asarray(labels)
    return np.asarray([normalized_edit_distance(h, labels[b, :int(label_len[b])]) for b, h in enumerate(hyp_rows)], dtype=np.float32)


def focal(loss, fl_gamma):
    """chiron_model.py:65-69: (1 - exp(-loss))^fl_gamma * loss, per row (float64)."""
    loss = np.asarray(loss, dtype=np.float64)
    return np.power(1.0 - np.exp(-loss), fl_gamma) * loss
