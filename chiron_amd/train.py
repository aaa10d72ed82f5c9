"""Fine-tuning of the recurrent stack and the FC head on the GPU, the CNN frozen: the reference's training loop
(chiron/chiron_rcnn_train.py:99-135: sess.run([net.ctc_loss, net.step]), validation every few steps, Saver.save) restricted to the
variables of rnn.py:20-174 and the head :72-96.

The forward pass with its tape and the backward pass are HIP kernels (csrc/rnn_grad.hip, chiron_rnn_train_forward /
chiron_rnn_train_backward); the loss gradient is chiron_ctc_loss (ctc.CTCLoss); torch owns the memory, the autograd graph and the
optimizer.  There is no CPU fallback.

The trainable parameter vector is one flat float32 tensor: the slice of the engine's weight blob from the first lstm_cell/kernel
to rnn_fnn_layer/bias_class (chiron_rnn_params_range), in that layout; `named_views` gives the TF variables as views into it.
"""
import ctypes as C
import json
import logging
import os
from collections import OrderedDict

import numpy as np

from . import _lib

logger = logging.getLogger(__name__)

OPT_METHODS = ("Adam", "SGD", "RMSProp", "Momentum")   # chiron_model.py:77-99 train_opt


def _torch():
    import torch
    return torch


def params_range(spec):
    """(first float, float count) of the recurrent-plus-head section of the weight blob (chiron_rnn_params_range)."""
    return _lib.sized2("chiron_rnn_params_range", C.byref(spec.to_c()))


def train_sizes(spec, batch, T):
    """(tape bytes, workspace bytes) of one batch (chiron_rnn_train_sizes).  Host-only."""
    return _lib.sized2("chiron_rnn_train_sizes", C.byref(spec.to_c()), int(batch), int(T))


def param_layout(spec):
    """Ordered {TF variable name: (offset in the parameter vector, shape)} of the trainable slice."""
    out, off = OrderedDict(), 0
    for name, shape in spec._rnn_and_head():
        out[name] = (off, tuple(shape))
        off += int(np.prod(shape))
    return out


def _device_index(t):
    torch = _torch()
    return t.device.index if t.device.index is not None else torch.cuda.current_device()


def rnn_forward(spec, params, features, seq_len):
    """chiron_rnn_train_forward on torch CUDA tensors (float32 params [n], features [B, T, C], int32 seq_len [B], all contiguous)
    -> (logits [B, T, 5], tape, workspace); enqueued on the current stream."""
    torch = _torch()
    B, T, _ = features.shape
    tape_b, ws_b = train_sizes(spec, B, T)
    dev = features.device
    logits = _lib.device_output((B, T, _lib.CLASSES), torch.float32, dev)
    tape = _lib.device_bytes(tape_b, dev)
    ws = _lib.device_bytes(ws_b, dev)
    desc = spec.to_c()
    _lib.check(_lib.load().chiron_rnn_train_forward(_device_index(features), C.byref(desc), params.data_ptr(), features.data_ptr(),
                                                    seq_len.data_ptr(), B, T, logits.data_ptr(), tape.data_ptr(), ws.data_ptr(),
                                                    C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return logits, tape, ws


def rnn_backward(spec, params, features, seq_len, dlogits, tape, ws, want_dfeatures=True):
    """chiron_rnn_train_backward -> (dparams [n], dfeatures [B, T, C] or None)."""
    torch = _torch()
    B, T, _ = features.shape
    dev = features.device
    dparams = _lib.device_output(params.shape, params.dtype, params.device)
    dfeat = _lib.device_output(features.shape, features.dtype, dev) if want_dfeatures else None
    desc = spec.to_c()
    _lib.check(_lib.load().chiron_rnn_train_backward(_device_index(features), C.byref(desc), params.data_ptr(), features.data_ptr(),
                                                     seq_len.data_ptr(), dlogits.data_ptr(), B, T, tape.data_ptr(), ws.data_ptr(),
                                                     dparams.data_ptr(), dfeat.data_ptr() if want_dfeatures else None,
                                                     C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return dparams, dfeat


def _check_inputs(params, features, seq_len):
    torch = _torch()
    if not (features.is_cuda and params.is_cuda):
        raise ValueError("features and parameters must be CUDA tensors: the training kernels have no CPU fallback")
    if features.dim() != 3:
        raise ValueError("features must be [batch, T, C]")
    features = features.to(torch.float32).contiguous()
    seq_len = seq_len.to(device=features.device, dtype=torch.int32).contiguous()
    if seq_len.shape != (features.shape[0],):
        raise ValueError("seq_len must be [batch]")
    return features, seq_len


_FN = None


def _function():
    global _FN
    if _FN is not None:
        return _FN
    torch = _torch()

    class RnnHeadFunction(torch.autograd.Function):
        """logits = f(params, features, seq_len, spec): forward with a tape, backward through the HIP BPTT."""

        @staticmethod
        def forward(ctx, params, features, seq_len, spec):
            p = params.detach().contiguous()
            logits, tape, ws = rnn_forward(spec, p, features, seq_len)
            ctx.spec = spec
            ctx.tape, ctx.ws = tape, ws
            ctx.save_for_backward(p, features, seq_len)
            return logits

        @staticmethod
        def backward(ctx, dlogits):
            p, features, seq_len = ctx.saved_tensors
            dparams, dfeat = rnn_backward(ctx.spec, p, features, seq_len, dlogits.to(torch.float32).contiguous(), ctx.tape, ctx.ws,
                                          want_dfeatures=ctx.needs_input_grad[1])
            ctx.tape = ctx.ws = None
            return dparams, dfeat, None, None

    _FN = RnnHeadFunction
    return _FN


class RecurrentHead(object):
    """torch.nn.Module over the recurrent stack and the FC head of `spec`: one flat float32 CUDA parameter `flat` (the blob slice of
    chiron_rnn_params_range, initialised from `weights`), forward(features [B, T, C], seq_len [B]) -> logits [B, T, 5].  The module
    class is built on first use so that importing this file needs no torch."""

    def __new__(cls, spec, weights, device=None):
        return _recurrent_head_class()(spec, weights, device)


_RH = None


def _recurrent_head_class():
    global _RH
    if _RH is not None:
        return _RH
    torch = _torch()

    class _RecurrentHead(torch.nn.Module):
        def __init__(self, spec, weights, device=None):
            torch.nn.Module.__init__(self)
            self.spec = spec
            first, n = params_range(spec)
            blob = spec.pack(weights)
            if first + n != blob.size:
                raise ValueError("the recurrent section does not end the weight blob")
            self.layout = param_layout(spec)
            self._frozen = OrderedDict((k, np.array(v, dtype=np.float32)) for k, v in spec.canonical_weights(weights).items()
                                       if k not in self.layout)
            dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
            self.flat = torch.nn.Parameter(torch.from_numpy(blob[first:first + n].copy()).to(dev))

        def named_views(self, tensor=None):
            """Ordered {TF variable name: view} into the parameter (or into `tensor`, e.g. its .grad)."""
            t = self.flat if tensor is None else tensor
            return OrderedDict((name, t[off:off + int(np.prod(shape))].view(*shape)) for name, (off, shape) in self.layout.items())

        def forward(self, features, seq_len):
            features, seq_len = _check_inputs(self.flat, features, seq_len)
            return _function().apply(self.flat, features, seq_len, self.spec)

        def state_weights(self):
            """The full weights dict: the frozen CNN entries plus the current parameters, ready for Engine(spec, weights, ...)."""
            out = OrderedDict(self._frozen)
            host = self.flat.detach().cpu().numpy()
            for name, (off, shape) in self.layout.items():
                out[name] = host[off:off + int(np.prod(shape))].reshape(shape).copy()
            return self.spec.canonical_weights(out)

    _RH = _RecurrentHead
    return _RH


def device_features(engine, slot=0):
    """The CNN feature tensor of the batch last collected on `slot` as a torch CUDA tensor of its own: one device-to-device copy of
    the engine's buffer (chiron_engine_device_features), no host round trip."""
    torch = _torch()
    ptr, b, c = engine.device_features(slot)

    class _View(object):
        __cuda_array_interface__ = {"shape": (b, engine.T, c), "typestr": "<f4", "data": (ptr, False), "version": 2, "strides": None}

    return torch.as_tensor(_View(), device=torch.device("cuda", engine.device_id)).clone()


def clip_by_norm_(views, clip):
    """tf.clip_by_norm on every variable's gradient (chiron_rcnn_train.py:55-57): g * clip / max(||g||, clip), in place."""
    torch = _torch()
    for g in views.values():
        g.mul_(clip / torch.clamp(torch.linalg.vector_norm(g), min=clip))


def make_optimizer(name, params, step_rate):
    """chiron_model.py:77-99 train_opt by name, through torch.optim."""
    torch = _torch()
    if name == "Adam":
        return torch.optim.Adam(params, lr=step_rate)
    if name == "SGD":
        return torch.optim.SGD(params, lr=step_rate)
    if name == "RMSProp":
        return torch.optim.RMSprop(params, lr=step_rate, alpha=0.9, eps=1e-10)
    if name == "Momentum":
        return torch.optim.SGD(params, lr=step_rate, momentum=0.9)
    raise ValueError("opt_method %r: one of %s" % (name, ", ".join(OPT_METHODS)))


def batch_loss(logits, seq_len, labels, label_len, fl_gamma=0.0):
    """chiron_model.loss (chiron_model.py:50-75): per-row CTC loss, the focal weight (1 - exp(-loss))^gamma when fl_gamma > 0
    (:64-69), then the mean; infeasible rows (loss +inf, where TF raises) are masked out, as `validate` leaves them out."""
    torch = _torch()
    from . import ctc
    loss = ctc.CTCLoss.apply(logits, seq_len, labels, label_len)
    kept = torch.isfinite(loss)
    loss = torch.where(kept, loss, torch.zeros_like(loss))
    if fl_gamma > 0:
        loss = torch.pow(torch.clamp(1.0 - torch.exp(-loss), min=0.0), fl_gamma) * loss
    return loss.sum() / torch.clamp(kept.sum(), min=1)


def save_model(out_dir, spec, weights, step, config):
    """<out>/model.json, checkpoint and final.ckpt-<step>.{index,data-00000-of-00001} (chiron_rcnn_train.py:110-113, :134), loadable
    through model.load_model, under the variable names of the model's own BN naming (ModelSpec.variables())."""
    from . import tf_bundle
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "model.json"), "w") as f:
        json.dump(config, f)
    canon = spec.canonical_weights(weights)
    # a batch-BN model (cnn.py:181-186 naming) stores scale and offset under its own names and no statistics
    alias = {}
    for site, _, has_bn in spec._sites():
        if has_bn:
            alias.update((name, site + "_bn/" + leaf) for leaf, name in zip(spec.BN_LEAVES, spec.bn_names(site)) if name is not None)
    tensors = OrderedDict((name, np.asarray(canon[alias.get(name, name)], dtype=np.float32).reshape(shape))
                          for name, shape in spec.variables().items())
    tensors["global_step"] = np.asarray(step, dtype=np.int64)
    name = "final.ckpt-%d" % step
    tf_bundle.write_bundle(os.path.join(out_dir, name), tensors)
    tf_bundle.write_checkpoint_file(out_dir, name)
    return os.path.join(out_dir, name)


def config_for(spec, base=None, opt_method="Adam", fl_gamma=0.0):
    """model.json of the saved model: the input model's, with the optimizer and focal gamma of this run (chiron_model.py:37-48)."""
    config = dict(base) if base else {"cnn": {"model": "dna_model1" if spec.rnn_kind == "stack" else "rna_model3"}}
    config["rnn"] = {"layer_num": spec.rnn_layers, "hidden_num": spec.hidden, "cell_type": "LSTM",
                     "layer_type": "rna" if spec.rnn_kind == "multi" else "normal"}
    config["opt_method"] = opt_method
    config["fl_gamma"] = fl_gamma
    return config


def finetune(args):
    """The loop of chiron_rcnn_train.py:99-135 restricted to the recurrent stack and the head.

    Windows come from labelled.read_raw_data_sets (-i; -v for validation, else the training windows), shuffled by --seed; features
    from a population-BN fp32 Engine (the frozen CNN) through chiron_engine_device_features; logits from RecurrentHead; the loss is
    `batch_loss` (ctc.CTCLoss, focal term when --fl_gamma > 0, mean over the feasible rows); --gradient_clip is tf.clip_by_norm per
    variable; the optimizer is one of train_opt's four names through torch.optim.  The optimizers' arithmetic is torch's, not
    pinned to TF's (epsilon placement, bias correction and RMSProp's accumulator differ in detail).  Every --report-every steps the
    training loss and the validation edit distance (a second Engine built from the current weights, Engine.score) are logged.
    Ends by writing <out>/model.json, checkpoint and final.ckpt-<step>.*, which `chiron call -m <out>` and `validate -m <out>` load.
    Returns the report dict (also written to <out>/finetune.json)."""
    torch = _torch()
    from . import labelled, model as model_mod
    from .engine import Engine, seq_len_for_engine
    if args.opt_method not in OPT_METHODS:
        raise ValueError("opt_method %r: one of %s" % (args.opt_method, ", ".join(OPT_METHODS)))
    torch.manual_seed(args.seed)
    rng = np.random.RandomState(args.seed)
    ds = labelled.read_raw_data_sets(args.input, seq_length=args.sequence_len, max_segments=args.segments_num, sig_norm=args.sig_norm)
    n = ds.event.shape[0]
    if n == 0:
        raise ValueError("no labelled window under %s" % args.input)
    vs = ds if not args.validation else labelled.read_raw_data_sets(args.validation, seq_length=args.sequence_len,
                                                                  max_segments=args.segments_num, sig_norm=args.sig_norm)
    spec, weights, config = model_mod.load_model(args.model, allow_synthetic=args.synthetic_weights)
    if spec.bn_mode != "population":
        raise ValueError("fine-tuning needs a population-BN model (the CNN is frozen)")
    bsz = min(args.batch_size, n)
    dev = torch.device("cuda", args.device)
    head = RecurrentHead(spec, weights, device=args.device)
    opt = make_optimizer(args.opt_method, [head.flat], args.step_rate)
    reports, window = [], []

    def validation_error(step_weights):
        nv = min(bsz, vs.event.shape[0])
        with Engine(spec, step_weights, max_batch=nv, segment_len=args.sequence_len, device_id=args.device) as ve:
            x = np.ascontiguousarray(vs.event[:nv], dtype=np.float32)
            sl = seq_len_for_engine(vs.event_length[:nv], ve.ratio)
            ve.submit(0, x, sl, beam_width=0, want_prob=False)
            ve.collect(0)
            _, edit, _ = ve.score(0, labelled.dense_labels(vs.label[:nv], vs.label_length[:nv]), vs.label_length[:nv])
        return float(np.mean(edit, dtype=np.float64))

    def to_dev(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)

    with Engine(spec, weights, max_batch=bsz, segment_len=args.sequence_len, device_id=args.device) as cnn:
        order, pos = rng.permutation(n), 0
        for step in range(1, args.max_steps + 1):
            if pos + bsz > n:          # next epoch: a new order (read_data_sets.next_batch reshuffles at the epoch's end)
                order, pos = rng.permutation(n), 0
            rows = order[pos:pos + bsz]
            pos += bsz
            sl = seq_len_for_engine(ds.event_length[rows], cnn.ratio)
            ll = ds.label_length[rows]
            dense = labelled.dense_labels([ds.label[i] for i in rows], ll)
            cnn.submit(0, np.ascontiguousarray(ds.event[rows], dtype=np.float32), sl, beam_width=0, want_prob=False)
            cnn.collect(0)
            sl_d = to_dev(sl, np.int32)
            logits = head(device_features(cnn, 0), sl_d)
            loss = batch_loss(logits, sl_d, to_dev(dense, np.int32), to_dev(ll, np.int32), args.fl_gamma)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            if args.gradient_clip is not None:
                clip_by_norm_(head.named_views(head.flat.grad), float(args.gradient_clip))
            opt.step()
            window.append(float(loss.item()))
            if step % args.report_every == 0 or step == args.max_steps:
                rep = {"step": step, "train_loss": float(np.mean(window)), "validation_error": validation_error(head.state_weights())}
                window = []
                reports.append(rep)
                logger.info("Step %d, loss %.5f, edit_distance %.5f", step, rep["train_loss"], rep["validation_error"])
    prefix = save_model(args.output, spec, head.state_weights(), args.max_steps, config_for(spec, config, args.opt_method, args.fl_gamma))
    report = {"input": args.input, "model": args.model, "checkpoint": prefix, "steps": args.max_steps, "batch_size": bsz,
              "windows": int(n), "opt_method": args.opt_method, "step_rate": args.step_rate, "reports": reports}
    with open(os.path.join(args.output, "finetune.json"), "w") as f:
        json.dump(report, f, indent=1)
    return report


# ---------------------------------------------------------------------------------------------
# the whole network: CNN seam + recurrent seam, `chiron train`
# ---------------------------------------------------------------------------------------------
BN_DECAY = 0.99   # cnn.py:125 batchnorm(decay=0.99)


def cnn_params_range(spec):
    """(first float, float count) of the CNN section of the weight blob (chiron_cnn_params_range)."""
    return _lib.sized2("chiron_cnn_params_range", C.byref(spec.to_c()))


def cnn_train_sizes(spec, batch, segment_len):
    """(tape bytes, workspace bytes) of one batch (chiron_cnn_train_sizes).  Host-only."""
    return _lib.sized2("chiron_cnn_train_sizes", C.byref(spec.to_c()), int(batch), int(segment_len))


def cnn_param_layout(spec):
    """Ordered {canonical name: (offset in the CNN section, shape)}: the entries of blob_layout() before the first lstm_cell/kernel."""
    rnn = set(name for name, _ in spec._rnn_and_head())
    out, off = OrderedDict(), 0
    for name, shape in spec.blob_layout().items():
        if name in rnn:
            break
        out[name] = (off, tuple(shape))
        off += int(np.prod(shape))
    return out


def cnn_forward(spec, params, signal):
    """chiron_cnn_train_forward on torch CUDA tensors (float32 params [n], signal [B, L], contiguous) -> (features [B, T, C], moments
    [n] with the pop_mean / pop_var slots holding the batch's mean / biased variance and zeros elsewhere, tape, workspace)."""
    torch = _torch()
    B, L = signal.shape
    tape_b, ws_b = cnn_train_sizes(spec, B, L)
    dev = signal.device
    feats = _lib.device_output((B, spec.output_len(L), spec.blocks[-1]["out"]), torch.float32, dev)
    moments = torch.zeros_like(params)
    tape = _lib.device_bytes(tape_b, dev)
    ws = _lib.device_bytes(ws_b, dev)
    desc = spec.to_c()
    _lib.check(_lib.load().chiron_cnn_train_forward(_device_index(signal), C.byref(desc), params.data_ptr(), signal.data_ptr(), B, L,
                                                    feats.data_ptr(), moments.data_ptr(), tape.data_ptr(), ws.data_ptr(),
                                                    C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return feats, moments, tape, ws


def cnn_tape_relu(spec, tape, batch, segment_len):
    """Ordered {name: float32 view [batch, frames, channels] into `tape`} of the ReLU outputs the forward kept
    (chiron_cnn_train_tape_relu): the stem's site name, per block <block>/branch2/conv2a, <block>/branch2/conv2b and <block>/out.
    `view > 0` is the mask the backward uses."""
    torch = _torch()
    names = ([spec.STEM_SITE] if spec.stem else []) + [b["name"] + leaf for b in spec.blocks
                                                        for leaf in ("/branch2/conv2a", "/branch2/conv2b", "/out")]
    floats = tape.view(torch.float32)
    desc = spec.to_c()
    out = OrderedDict()
    for i, name in enumerate(names):
        off, frames, ch = C.c_size_t(), C.c_int32(), C.c_int32()
        _lib.check(_lib.load().chiron_cnn_train_tape_relu(C.byref(desc), int(batch), int(segment_len), i, C.byref(off), C.byref(frames),
                                                          C.byref(ch)))
        n = int(batch) * frames.value * ch.value
        out[name] = floats[off.value:off.value + n].view(int(batch), frames.value, ch.value)
    return out


def cnn_backward(spec, params, signal, dfeatures, tape, ws):
    """chiron_cnn_train_backward -> dparams [n] (exactly 0 in the pop_mean / pop_var slots)."""
    torch = _torch()
    B, L = signal.shape
    dparams = _lib.device_output(params.shape, params.dtype, params.device)
    desc = spec.to_c()
    _lib.check(_lib.load().chiron_cnn_train_backward(_device_index(signal), C.byref(desc), params.data_ptr(), signal.data_ptr(),
                                                     dfeatures.data_ptr(), B, L, tape.data_ptr(), ws.data_ptr(), dparams.data_ptr(),
                                                     C.c_void_p(torch.cuda.current_stream(signal.device).cuda_stream)))
    return dparams


_NET_FN = None


def _network_function():
    global _NET_FN
    if _NET_FN is not None:
        return _NET_FN
    torch = _torch()

    class NetworkFunction(torch.autograd.Function):
        """(logits, moments) = f(flat, signal, seq_len, spec): the CNN seam chained into the recurrent seam with no copy; backward
        runs chiron_rnn_train_backward, hands its dfeatures to chiron_cnn_train_backward and returns the two sections side by side."""

        @staticmethod
        def forward(ctx, flat, signal, seq_len, spec):
            p = flat.detach().contiguous()
            n_cnn = cnn_params_range(spec)[1]
            pc, pr = p[:n_cnn], p[n_cnn:]
            feats, moments, ctape, cws = cnn_forward(spec, pc, signal)
            logits, rtape, rws = rnn_forward(spec, pr, feats, seq_len)
            ctx.spec, ctx.n_cnn = spec, n_cnn
            ctx.tapes = (ctape, cws, rtape, rws)
            ctx.save_for_backward(p, signal, seq_len, feats)
            ctx.mark_non_differentiable(moments)
            return logits, moments

        @staticmethod
        def backward(ctx, dlogits, _dmoments):
            p, signal, seq_len, feats = ctx.saved_tensors
            ctape, cws, rtape, rws = ctx.tapes
            pc, pr = p[:ctx.n_cnn], p[ctx.n_cnn:]
            d_rnn, dfeat = rnn_backward(ctx.spec, pr, feats, seq_len, dlogits.to(torch.float32).contiguous(), rtape, rws, True)
            d_cnn = cnn_backward(ctx.spec, pc, signal, dfeat, ctape, cws)
            ctx.tapes = None
            return torch.cat([d_cnn, d_rnn]), None, None, None

    _NET_FN = NetworkFunction
    return _NET_FN


class Network(object):
    """torch.nn.Module over the whole network of `spec`: one flat float32 CUDA parameter `flat` in the weight blob's layout
    (ModelSpec.blob_layout(): the CNN section, then the recurrent section that RecurrentHead owns), forward(signal [B, L],
    seq_len [B]) -> logits [B, T, 5].  Batch normalisation uses the batch's moments in every forward (training semantics); in
    train() mode each forward also moves the statistics: pop = 0.99 * pop + 0.01 * batch (cnn.py:153-156, biased variance).  The
    pop_mean / pop_var slots get a zero gradient.  The module class is built on first use so that importing this file needs no torch."""

    def __new__(cls, spec, weights, device=None):
        return _network_class()(spec, weights, device)


_NET = None


def _network_class():
    global _NET
    if _NET is not None:
        return _NET
    torch = _torch()

    class _Network(torch.nn.Module):
        def __init__(self, spec, weights, device=None):
            torch.nn.Module.__init__(self)
            self.spec = spec
            blob = spec.pack(weights)
            (c0, cn), (r0, rn) = cnn_params_range(spec), params_range(spec)
            if c0 != 0 or r0 != cn or r0 + rn != blob.size:
                raise ValueError("the CNN and the recurrent sections do not tile the weight blob")
            self.layout, off = OrderedDict(), 0
            for name, shape in spec.blob_layout().items():
                self.layout[name] = (off, tuple(shape))
                off += int(np.prod(shape))
            dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
            self.flat = torch.nn.Parameter(torch.from_numpy(blob.copy()).to(dev))
            stat = np.concatenate([np.arange(o, o + int(np.prod(sh))) for name, (o, sh) in self.layout.items()
                                   if name.endswith(("_bn/pop_mean", "_bn/pop_var"))])
            self.register_buffer("stat_index", torch.from_numpy(stat).to(dev), persistent=False)
            self.last_moments = None

        def named_views(self, tensor=None):
            """Ordered {canonical variable name: view} into the parameter (or into `tensor`, e.g. its .grad)."""
            t = self.flat if tensor is None else tensor
            return OrderedDict((name, t[off:off + int(np.prod(shape))].view(*shape)) for name, (off, shape) in self.layout.items())

        def forward(self, signal, seq_len):
            if not (signal.is_cuda and signal.dim() == 2):
                raise ValueError("signal must be a CUDA tensor [batch, segment_len]: the training kernels have no CPU fallback")
            signal = signal.to(torch.float32).contiguous()
            seq_len = seq_len.to(device=signal.device, dtype=torch.int32).contiguous()
            if seq_len.shape != (signal.shape[0],):
                raise ValueError("seq_len must be [batch]")
            logits, moments = _network_function().apply(self.flat, signal, seq_len, self.spec)
            self.last_moments = moments
            if self.training:
                # the tensor saved for backward aliases `flat`; changing the statistics' slots under it is harmless because neither
                # chiron_cnn_train_forward nor _backward reads them
                with torch.no_grad():
                    idx = self.stat_index
                    self.flat.data[idx] = BN_DECAY * self.flat.data[idx] + (1.0 - BN_DECAY) * moments[idx]
            return logits

        def state_weights(self):
            """The full canonical weights dict of the current parameters, ready for Engine(spec, weights, ...) and save_model."""
            host = self.flat.detach().cpu().numpy()
            return OrderedDict((name, host[off:off + int(np.prod(shape))].reshape(shape).copy()) for name, (off, shape) in self.layout.items())

    _NET = _Network
    return _NET


def _truncated_normal(rng, stddev, shape):
    """tf.truncated_normal: N(0, stddev^2) redrawn outside two standard deviations."""
    out = rng.normal(0.0, stddev, shape)
    bad = np.abs(out) > 2.0 * stddev
    while bad.any():
        out[bad] = rng.normal(0.0, stddev, int(bad.sum()))
        bad = np.abs(out) > 2.0 * stddev
    return out.astype(np.float32)


def init_weights(spec, seed=1234):
    """From-scratch weights under the canonical names of spec.blob_layout(), following the reference's initialisers IN DISTRIBUTION;
    numpy's random stream, not TF's: no draw is bit-compatible with a TF run.

    - convolution filters (cnn.py:42-45): tf.contrib.layers.xavier_initializer(uniform=False) = truncated normal (two sigma) of
      pre-truncation deviation sqrt(1.3 * 2 / (fan_in + fan_out)), fan = k * channels: a sample deviation of sqrt(2 / (fan_in + fan_out));
    - population-BN sites (cnn.py:141-148): scale = 0.1; offset = tf.get_variable's default, Glorot uniform on [size]: U(+-sqrt(3 / size));
      pop_mean = 0, pop_var = 1;
    - batch-BN sites (cnn.py:181-186): scale and offset both tf.contrib.layers.variance_scaling_initializer() (factor 2, fan-in,
      truncated normal): pre-truncation deviation sqrt(1.3 * 2 / size) around ZERO; the statistics' slots hold 0 / 1 and are not saved;
    - lstm_cell/kernel: LSTMCell's default, Glorot uniform U(+-sqrt(6 / (rows + 4 H))); lstm_cell/bias = 0;
    - head (rnn.py:72-96): weights tf.truncated_normal_initializer(stddev=sqrt(2 / (2 H))), weights_class stddev sqrt(2 / H)
      (pre-truncation deviations), both biases 0."""
    rng = np.random.RandomState(seed)
    H = spec.hidden
    w = OrderedDict()
    for site, shape, has_bn in spec._sites():
        _, k, ci, co = shape
        w[site + "/weights"] = _truncated_normal(rng, np.sqrt(1.3 * 2.0 / (k * ci + k * co)), shape)
        if not has_bn:
            continue
        if spec.bn_mode == "population":
            w[site + "_bn/scale"] = np.full(co, 0.1, dtype=np.float32)
            lim = np.sqrt(3.0 / co)
            w[site + "_bn/offset"] = rng.uniform(-lim, lim, co).astype(np.float32)
        else:
            w[site + "_bn/scale"] = _truncated_normal(rng, np.sqrt(1.3 * 2.0 / co), (co,))
            w[site + "_bn/offset"] = _truncated_normal(rng, np.sqrt(1.3 * 2.0 / co), (co,))
        w[site + "_bn/pop_mean"] = np.zeros(co, dtype=np.float32)
        w[site + "_bn/pop_var"] = np.ones(co, dtype=np.float32)
    for l in range(spec.rnn_layers):
        for d in ("fw", "bw"):
            rows = spec.lstm_in_width(l) + H
            lim = np.sqrt(6.0 / (rows + 4 * H))
            w[spec.lstm_scope(l, d) + "kernel"] = rng.uniform(-lim, lim, (rows, 4 * H)).astype(np.float32)
            w[spec.lstm_scope(l, d) + "bias"] = np.zeros(4 * H, dtype=np.float32)
    w["rnn_fnn_layer/weights"] = _truncated_normal(rng, np.sqrt(2.0 / (2 * H)), (2, H))
    w["rnn_fnn_layer/bias"] = np.zeros(H, dtype=np.float32)
    w["rnn_fnn_layer/weights_class"] = _truncated_normal(rng, np.sqrt(2.0 / H), (H, spec.classes))
    w["rnn_fnn_layer/bias_class"] = np.zeros(spec.classes, dtype=np.float32)
    return OrderedDict((k, w[k]) for k in spec.blob_layout())


def _checkpoint_step(model_dir):
    from . import tf_bundle
    prefix = tf_bundle.latest_checkpoint(model_dir)
    if prefix is None or not os.path.exists(prefix + ".index"):
        return 0
    entries = tf_bundle.read_index(prefix + ".index")
    if "global_step" not in entries:
        return 0
    return int(tf_bundle.read_tensors(prefix, entries, ["global_step"])["global_step"])


def train_network(args):
    """The loop of chiron_rcnn_train.py:99-135 on every variable of cnn.py and rnn.py: `finetune`'s loop with Network in place of
    engine + RecurrentHead.

    The start: -m given, that model (either BN naming); --retrain, the newest checkpoint under -o with its global_step carried on
    (the optimizer's state is NOT in a checkpoint written here: it restarts); neither, init_weights of the topology that --configure
    (a model.json; default chiron_model.py:37-48's) names, with --bn batch (what HEAD builds) or population.  Batch normalisation
    uses the batch's moments in every training step whatever the model's BN naming; a population-BN model's statistics move by
    0.99 / 0.01 each step and are saved, a batch-BN model's are not saved.  Validation builds a second Engine from the current
    weights in the model's own bn_mode (the reference validates with training=True, chiron_rcnn_train.py:116; that is not
    reproduced).  Writes <out>/model.json, checkpoint, final.ckpt-<step>.* and train.json; returns the report dict."""
    torch = _torch()
    from . import labelled, model as model_mod
    from .engine import Engine, seq_len_for_engine
    if args.opt_method not in OPT_METHODS:
        raise ValueError("opt_method %r: one of %s" % (args.opt_method, ", ".join(OPT_METHODS)))
    torch.manual_seed(args.seed)
    rng = np.random.RandomState(args.seed)
    ds = labelled.read_raw_data_sets(args.input, seq_length=args.sequence_len, max_segments=args.segments_num, sig_norm=args.sig_norm)
    n = ds.event.shape[0]
    if n == 0:
        raise ValueError("no labelled window under %s" % args.input)
    vs = ds if not args.validation else labelled.read_raw_data_sets(args.validation, seq_length=args.sequence_len,
                                                                  max_segments=args.segments_num, sig_norm=args.sig_norm)
    step0 = 0
    if args.retrain:
        spec, weights, config = model_mod.load_model(args.output)
        step0 = _checkpoint_step(args.output)
    elif args.model:
        spec, weights, config = model_mod.load_model(args.model, allow_synthetic=args.synthetic_weights)
    else:
        config = model_mod.read_config(args.configure)
        spec = model_mod.spec_from_config(config, args.bn)
        weights = init_weights(spec, args.seed)
    bsz = min(args.batch_size, n)
    dev = torch.device("cuda", args.device)
    net = Network(spec, weights, device=args.device)
    net.train()
    opt = make_optimizer(args.opt_method, [net.flat], args.step_rate)
    ratio = float(args.sequence_len) / spec.output_len(args.sequence_len)
    reports, window = [], []

    def validation_error(step_weights):
        nv = min(bsz, vs.event.shape[0])
        with Engine(spec, step_weights, max_batch=nv, segment_len=args.sequence_len, device_id=args.device) as ve:
            x = np.ascontiguousarray(vs.event[:nv], dtype=np.float32)
            sl = seq_len_for_engine(vs.event_length[:nv], ve.ratio)
            ve.submit(0, x, sl, beam_width=0, want_prob=False)
            ve.collect(0)
            _, edit, _ = ve.score(0, labelled.dense_labels(vs.label[:nv], vs.label_length[:nv]), vs.label_length[:nv])
        return float(np.mean(edit, dtype=np.float64))

    def to_dev(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)

    order, pos = rng.permutation(n), 0
    for step in range(1, args.max_steps + 1):
        if pos + bsz > n:
            order, pos = rng.permutation(n), 0
        rows = order[pos:pos + bsz]
        pos += bsz
        sl = seq_len_for_engine(ds.event_length[rows], ratio)
        ll = ds.label_length[rows]
        dense = labelled.dense_labels([ds.label[i] for i in rows], ll)
        sl_d = to_dev(sl, np.int32)
        logits = net(to_dev(ds.event[rows], np.float32), sl_d)
        loss = batch_loss(logits, sl_d, to_dev(dense, np.int32), to_dev(ll, np.int32), args.fl_gamma)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        if args.gradient_clip is not None:
            clip_by_norm_(net.named_views(net.flat.grad), float(args.gradient_clip))
        opt.step()
        window.append(float(loss.item()))
        if step % args.report_every == 0 or step == args.max_steps:
            rep = {"step": step0 + step, "train_loss": float(np.mean(window)), "validation_error": validation_error(net.state_weights())}
            window = []
            reports.append(rep)
            logger.info("Step %d, loss %.5f, edit_distance %.5f", rep["step"], rep["train_loss"], rep["validation_error"])
    final = step0 + args.max_steps
    prefix = save_model(args.output, spec, net.state_weights(), final, config_for(spec, config, args.opt_method, args.fl_gamma))
    report = {"input": args.input, "model": args.model, "checkpoint": prefix, "steps": args.max_steps, "global_step": final,
              "batch_size": bsz, "windows": int(n), "bn_mode": spec.bn_mode, "opt_method": args.opt_method, "step_rate": args.step_rate,
              "reports": reports}
    with open(os.path.join(args.output, "train.json"), "w") as f:
        json.dump(report, f, indent=1)
    return report
