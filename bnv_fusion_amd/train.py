"""Training of the local shape embedding (point encoder + SDF decoder) on the GPU: the reference's
``LitFusionPointNet.training_step`` with ``training_global=False`` (local_point_fusion.py:381-460, src/train.py).

One ``EmbeddingTrainer.step`` is ONE call into the shared library (csrc/train.hip, include/bnv_fusion.h:
bnv_train_step): encoder forward with train-mode BatchNorm, decoder forward, loss, the gradient of every parameter,
the running-stat update and an Adam step, all on the caller's stream, in exact fp32, with every row sum reduced in a
fixed order -- a run is bit-reproducible.  The parameters live on the device in one flat buffer in state_dict order;
``state_dict()`` / ``save_npz`` / ``save_ckpt`` / ``to_model`` hand them to the inference side.

Stated differences from the reference: fp32 instead of fp16 AMP; the number of input points per step
``n`` is drawn from the trainer's own seeded generator instead of torch's global RNG; reductions run in a fixed order.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib

N_LOCAL_SAMPLES = 64        # fusion_pointnet_dataset.yaml: n_local_samples
MIN_PTS_IN_GRID = 8         # fusion_pointnet_model.yaml: min_pts_in_grid; a step draws n in [min_pts / 2, 64)
LOSS_WEIGHTS = {"bce_loss": 1.0, "reg_loss": 0.001}   # fusion_pointnet_model.yaml:36-38 (fixed in the kernels)
LR_STEP_SIZE, LR_GAMMA = 20000, 0.5                   # configs/optimizer/adam.yaml: StepLR, interval epoch

_CONV = [(6, 128), (128, 128), (128, 128), (128, 8)]
_GEO = [(17, 256), (256, 256), (256, 256), (256, 256)]

# trainable tensors in the order of the flat device buffer (include/bnv_fusion.h: bnv_train_step)
PARAM_SHAPES = (
    [(f"pointnet_backbone.conv{i + 1}.{p}", (o, c, 1) if p == "weight" else (o,))
     for i, (c, o) in enumerate(_CONV) for p in ("weight", "bias")]
    + [(f"pointnet_backbone.bn{i + 1}.{p}", (o,)) for i, (_, o) in enumerate(_CONV) for p in ("weight", "bias")]
    + [(f"nerf.geo_layer{i}.{p}", (o, c) if p == "weight" else (o,))
       for i, (c, o) in enumerate(_GEO) for p in ("weight", "bias")]
    + [("nerf.fc_alpha.weight", (1, 256)), ("nerf.fc_alpha.bias", (1,))])
# running statistics, per BatchNorm layer: running_mean then running_var
RUNNING_SHAPES = [(f"pointnet_backbone.bn{i + 1}.{p}", (o,)) for i, (_, o) in enumerate(_CONV)
                  for p in ("running_mean", "running_var")]
# the reference's colour head: in its state_dict (strict loading), never evaluated (modules.py:912-920)
COLOR_HEAD_SHAPES = [("nerf.color_layer0.weight", (128, 295)), ("nerf.color_layer0.bias", (128,)),
                     ("nerf.color_layer1.weight", (128, 128)), ("nerf.color_layer1.bias", (128,)),
                     ("nerf.fc_rgb.weight", (3, 128)), ("nerf.fc_rgb.bias", (3,))]


def state_dict_keys():
    """Keys of weights/pointnet_fp32.npz, in its order."""
    keys = [f"pointnet_backbone.conv{i + 1}.{p}" for i in range(4) for p in ("weight", "bias")]
    for i in range(4):
        keys += [f"pointnet_backbone.bn{i + 1}.{p}"
                 for p in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
    keys += [f"nerf.geo_layer{i}.{p}" for i in range(4) for p in ("weight", "bias")]
    return keys + ["nerf.fc_alpha.weight", "nerf.fc_alpha.bias"]


def default_state_dict(seed=0):
    """PyTorch's default initialisation of the reference's Conv1d / BatchNorm1d / Linear layers, from ``seed``."""
    g = torch.Generator().manual_seed(int(seed))
    sd = {}

    def uniform(shape, bound):
        return ((torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * bound).float().numpy()

    def linear(prefix, c_in, shape_w, c_out):
        # kaiming_uniform_(a=sqrt(5)) on the weight and U(-1/sqrt(fan_in), 1/sqrt(fan_in)) on the bias: both bounds
        # are 1 / sqrt(fan_in)
        bound = 1.0 / np.sqrt(c_in)
        sd[prefix + ".weight"] = uniform(shape_w, bound)
        sd[prefix + ".bias"] = uniform((c_out,), bound)

    for i, (c, o) in enumerate(_CONV):
        linear(f"pointnet_backbone.conv{i + 1}", c, (o, c, 1), o)
    for i, (_, o) in enumerate(_CONV):
        p = f"pointnet_backbone.bn{i + 1}"
        sd[p + ".weight"] = np.ones(o, np.float32)
        sd[p + ".bias"] = np.zeros(o, np.float32)
        sd[p + ".running_mean"] = np.zeros(o, np.float32)
        sd[p + ".running_var"] = np.ones(o, np.float32)
        sd[p + ".num_batches_tracked"] = np.array(0, np.int64)
    for i, (c, o) in enumerate(_GEO):
        linear(f"nerf.geo_layer{i}", c, (o, c), o)
    linear("nerf.fc_alpha", 256, (1, 256), 1)
    return {k: sd[k] for k in state_dict_keys()}


def _np(v):
    return v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)


def _check_shapes(input_pts, training_pts, gt, n, batchnorm):
    """The shape guard of both trainers.  ``batchnorm``: the fp32 networks (B n >= 2); else the tiny-cuda-nn ones
    (B >= 1, B M <= 2^24)."""
    if input_pts.dim() != 3 or input_pts.shape[1] != N_LOCAL_SAMPLES or input_pts.shape[2] != 6 or \
            (not batchnorm and input_pts.shape[0] < 1):
        raise ValueError(f"input_pts must be [{'B' if batchnorm else 'B >= 1'}, {N_LOCAL_SAMPLES}, 6], "
                         f"got {tuple(input_pts.shape)}")
    B = input_pts.shape[0]
    if training_pts.dim() != 3 or training_pts.shape[0] != B or training_pts.shape[2] != 3:
        raise ValueError(f"training_pts must be [B={B}, M, 3], got {tuple(training_pts.shape)}")
    M = training_pts.shape[1]
    if tuple(gt.shape) not in ((B, M), (B, M, 1)):
        raise ValueError(f"gt must be [B={B}, M={M}], got {tuple(gt.shape)}")
    if not 1 <= n <= N_LOCAL_SAMPLES:
        raise ValueError(f"n={n}: 1 .. {N_LOCAL_SAMPLES} input points per patch")
    if batchnorm and B * n < 2:
        raise ValueError(f"B * n = {B * n}: train-mode BatchNorm needs at least two rows")
    if batchnorm and M < 1:
        raise ValueError("M must be >= 1")
    if not batchnorm and (M < 1 or B * M > (1 << 24)):
        raise ValueError(f"B * M = {B * M}: 1 .. 2^24 query points")
    return B, M


def check_shapes(input_pts, training_pts, gt, n):
    """ValueError unless input_pts [B, 64, 6], training_pts [B, M, 3], gt [B, M] (or [B, M, 1]), 1 <= n <= 64 and
    B n >= 2 (the batch statistics need two rows)."""
    return _check_shapes(input_pts, training_pts, gt, n, batchnorm=True)


def _require(sd, keys, shapes):
    """ValueError unless the initial weights ``sd`` hold every key of ``keys``, and ``shapes`` [(name, shape)] fit."""
    missing = [k for k in keys if k not in sd]
    if missing:
        raise ValueError(f"state_dict lacks {missing}")
    for k, shape in shapes:
        if tuple(np.shape(sd[k])) != shape:
            raise ValueError(f"{k}: shape {np.shape(sd[k])}, expected {shape}")


def _views(buf, shapes):
    """name -> view of a flat buffer (device tensor or numpy array) cut into ``shapes`` [(name, shape)], in order."""
    out, o = {}, 0
    for k, shape in shapes:
        size = int(np.prod(shape))
        out[k] = buf[o: o + size].reshape(shape)
        o += size
    return out


class _Trainer:
    """What the two trainers share: the flat device buffers of the weights and of Adam's state, the schedule, the
    draw of ``n``, the workspace and the call into the library.  A trainer names its tensors (``SHAPES``), its shape
    guard (``BATCHNORM``) and its entries (``ENTRY``: bnv_<ENTRY>_step and so on)."""
    SHAPES, BATCHNORM, ENTRY = None, None, None

    def __init__(self, sd, seed, lr, device, betas, eps):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"{type(self).__name__} runs on the GPU (device='cuda:<i>')")
        self.lib = _lib.require_device(self.device.index or 0)
        flat =np.concatenate([np.asarray(sd[k], np.float32).ravel() for k, _ in self.SHAPES])
        assert flat.size == int(getattr(self.lib, f"bnv_{self.ENTRY}_param_floats")())
        self.params = torch.from_numpy(flat).to(self.device)
        self.grads = torch.zeros_like(self.params)
        self.exp_avg = torch.zeros_like(self.params)
        self.exp_avg_sq = torch.zeros_like(self.params)
        self.base_lr, self.betas, self.eps = float(lr), tuple(float(b) for b in betas), float(eps)
        self.epoch = 0
        self.rng = np.random.default_rng(seed)
        self._ws = {}

    # ---- schedule ----
    @property
    def lr(self):
        """StepLR(step_size=20000, gamma=0.5) over epochs."""
        return self.base_lr * LR_GAMMA ** (self.epoch // LR_STEP_SIZE)

    def end_epoch(self):
        self.epoch += 1

    def draw_n(self):
        """n = randint(min_pts_in_grid / 2, n_local_samples), drawn once per step (local_point_fusion.py:411-415)."""
        return int(self.rng.integers(MIN_PTS_IN_GRID // 2, N_LOCAL_SAMPLES))

    # ---- calls ----
    def _workspace(self, B, M):
        """The workspace of the last (B, M), sized for the largest n; the library is asked on a miss only."""
        ws = self._ws.get((B, M))
        if ws is None:
            nbytes = int(getattr(self.lib, f"bnv_{self.ENTRY}_workspace_bytes")(B, N_LOCAL_SAMPLES, M))
            if nbytes == 0:
                raise ValueError(f"shape B={B}, M={M} out of range")
            ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._ws = {(B, M): ws}
        return ws

    def _inputs(self, input_pts, training_pts, gt, n):
        """The three inputs as contiguous fp32 device tensors, B, M and the workspace."""
        x, p, g = (torch.as_tensor(t).to(self.device, torch.float32).contiguous()
                   for t in (input_pts, training_pts, gt))
        B, M = _check_shapes(x, p, g, n, self.BATCHNORM)
        return x, p, g, B, M, self._workspace(B, M)

    def _call(self, what, *args):
        """bnv_<ENTRY>_<what>(tensors as pointers, scalars as they are, ..., stream) on this device; raises unless it
        succeeds."""
        name = f"bnv_{self.ENTRY}_{what}"
        with torch.cuda.device(self.device):
            rc = getattr(self.lib, name)(*[_lib.ptr(a) if torch.is_tensor(a) else a for a in args],
                                         _lib.stream_ptr())
        _lib.check(rc, name)

    def _adam_args(self):
        return [C.c_float(v) for v in (self.lr, self.betas[0], self.betas[1], self.eps)]

    # ---- weights out ----
    def parameters(self):
        """name -> device tensor view into the flat parameter buffer, in state_dict shapes."""
        return _views(self.params, self.SHAPES)

    def gradients(self):
        """name -> device tensor view of the last step's gradients."""
        return _views(self.grads, self.SHAPES)

    def save_npz(self, path):
        """Writes ``state_dict()`` in the layout of the shipped weights/pointnet_*.npz (``load_pretrained(path=...)``
        reads it; with ``tiny_cuda=True`` for the tiny-cuda-nn networks)."""
        with open(path, "wb") as fh:
            np.savez(fh, **self.state_dict())


class EmbeddingTrainer(_Trainer):
    """Trains the point encoder and SDF decoder with Adam (torch defaults, ``lr``) and an epoch-wise StepLR
    (step 20000, gamma 0.5), batch after batch, on ``device``.

    ``state_dict``: initial weights in the reference's key layout (``weights.load_npz``, a checkpoint's
    ``state_dict``); None: PyTorch's default initialisation from ``seed``.  ``seed`` also seeds the draw of ``n``."""
    SHAPES, BATCHNORM, ENTRY = PARAM_SHAPES, True, "train"

    def __init__(self, state_dict=None, seed=0, lr=1e-3, device="cuda:0", betas=(0.9, 0.999), eps=1e-8):
        sd = default_state_dict(seed) if state_dict is None else {k: _np(v) for k, v in state_dict.items()}
        _require(sd, state_dict_keys(), PARAM_SHAPES + RUNNING_SHAPES)
        super().__init__(sd, seed, lr, device, betas, eps)
        run = np.concatenate([np.asarray(sd[k], np.float32).ravel() for k, _ in RUNNING_SHAPES])
        assert run.size == int(self.lib.bnv_train_running_floats())
        self.running = torch.from_numpy(run).to(self.device)
        self.num_batches_tracked = [int(np.asarray(sd[f"pointnet_backbone.bn{i + 1}.num_batches_tracked"]))
                                    for i in range(4)]
        self.adam_step = 0

    def step(self, input_pts, training_pts, gt, n=None):
        """One training step on a batch: input_pts [B, 64, 6], training_pts [B, M, 3], gt [B, M].  The first ``n``
        points of every patch feed the encoder (None: drawn).  Returns the loss terms as device tensors
        ({"loss", "bce_loss", "reg_loss"}); nothing synchronises."""
        n = self.draw_n() if n is None else int(n)
        x, p, g, B, M, ws = self._inputs(input_pts, training_pts, gt, n)
        loss = torch.empty(3, dtype=torch.float32, device=self.device)
        self._call("step", self.params, self.grads, self.exp_avg, self.exp_avg_sq, self.running, x, p, g, B, n, M,
                   *self._adam_args(), self.adam_step + 1, loss, ws, ws.numel())
        self.adam_step += 1      # a failed call has raised: the step count stays as it was
        self.num_batches_tracked = [v + 1 for v in self.num_batches_tracked]
        return {"loss": loss[0], "bce_loss": loss[1], "reg_loss": loss[2]}

    def eval_loss(self, batch, n=N_LOCAL_SAMPLES):
        """Validation loss (local_point_fusion.py:462-480): eval-mode BatchNorm, all 64 points; returns the L1 term
        (``val_loss``) as a device scalar.  ``batch``: a dict with input_pts, training_pts, gt."""
        x, p, g, B, M, ws = self._inputs(batch["input_pts"], batch["training_pts"], batch["gt"], n)
        loss = torch.empty(3, dtype=torch.float32, device=self.device)
        self._call("eval_loss", self.params, self.running, x, p, g, B, n, M, loss, ws, ws.numel())
        return loss[1]

    def state_dict(self):
        """The weights as numpy arrays with exactly the keys, shapes and dtypes of weights/pointnet_fp32.npz."""
        sd = {k: v.copy() for k, v in _views(self.params.cpu().numpy(), PARAM_SHAPES).items()}
        sd.update({k: v.copy() for k, v in _views(self.running.cpu().numpy(), RUNNING_SHAPES).items()})
        for i in range(4):
            sd[f"pointnet_backbone.bn{i + 1}.num_batches_tracked"] = np.array(self.num_batches_tracked[i], np.int64)
        return {k: sd[k] for k in state_dict_keys()}

    def save_ckpt(self, path):
        """Writes ``{"state_dict": ...}`` that the reference's LitFusionPointNet loads strictly (run_e2e.py:232-233):
        the trained tensors plus the never-evaluated colour head as zeros."""
        sd = {k: torch.from_numpy(v) for k, v in self.state_dict().items()}
        for k, shape in COLOR_HEAD_SHAPES:
            sd[k] = torch.zeros(shape, dtype=torch.float32)
        torch.save({"state_dict": sd}, path)

    def to_model(self, voxel_size=0.01, min_pts_in_grid=MIN_PTS_IN_GRID, device=None):
        """A frozen LitFusionPointNet with these weights, repacked for the inference kernels (``NeuralMap``)."""
        from .fusion import load_pretrained
        return load_pretrained(device=device or self.device, voxel_size=voxel_size, min_pts_in_grid=min_pts_in_grid,
                               state_dict=self.state_dict())


# ---- the tiny-cuda-nn embedding (tiny_cuda: True, the reference's default) ----
TCNN_KEYS = ("pointnet_backbone.model.params", "nerf.model.params")
TCNN_WIDTHS = {"pointnet_backbone.model.params": (16, 64, 64, 64, 16), "nerf.model.params": (32, 64, 64, 64, 16)}
TCNN_SHAPES = [(k, (sum(a * b for a, b in zip(w[:-1], w[1:])),)) for k, w in TCNN_WIDTHS.items()]   # 10240, 11264


def tcnn_default_state_dict(seed=0):
    """Initial weights from ``seed``: Xavier-uniform per matrix, bound sqrt(6 / (fan_in + fan_out)) on the padded
    widths, drawn from torch.Generator(seed) as float64 U(-1, 1) * bound, encoder matrices then decoder matrices, each
    in layer order.  A documented replacement of tiny-cuda-nn's own initial_params stream, which cannot be reproduced
    (its FullyFusedMLP also initialises Xavier-uniform per matrix, from memory; unverified)."""
    g = torch.Generator().manual_seed(int(seed))
    sd = {}
    for k, w in TCNN_WIDTHS.items():
        mats = []
        for fan_in, fan_out in zip(w[:-1], w[1:]):
            bound = np.sqrt(6.0 / (fan_in + fan_out))
            mats.append(((torch.rand((fan_out, fan_in), generator=g, dtype=torch.float64) * 2 - 1) * bound).ravel())
        sd[k] = torch.cat(mats).float().numpy()
    return sd


def check_tcnn_shapes(input_pts, training_pts, gt, n):
    """ValueError unless input_pts [B, 64, 6], training_pts [B, M, 3], gt [B, M] (or [B, M, 1]), 1 <= n <= 64, M >= 1
    and B M <= 2^24 (no BatchNorm: B n = 1 is valid)."""
    return _check_shapes(input_pts, training_pts, gt, n, batchnorm=False)


class TcnnEmbeddingTrainer(_Trainer):
    """Trains the tiny-cuda-nn point encoder and SDF decoder (the reference's default, ``tiny_cuda: True``) with Adam
    and an epoch-wise StepLR, like ``EmbeddingTrainer``: csrc/train_tcnn.hip, include/bnv_fusion.h
    (bnv_train_tcnn_step).  Forward in the f16 arithmetic of MLP mode 2, backward straight-through with hi + lo f16
    gradient products, on the matrix cores.  A step whose loss or gradients are not finite is skipped on the device
    (the reference's AMP gradient scaler): ``step`` reports it in ``"skipped"``.

    ``state_dict``: initial weights with the two keys of weights/pointnet_tcnn.npz (``weights.load_npz(
    weights.DEFAULT_TCNN)`` fine-tunes the shipped checkpoint); None: ``tcnn_default_state_dict(seed)``.  ``seed`` also
    seeds the draw of ``n``."""

    SHAPES, BATCHNORM, ENTRY = TCNN_SHAPES, False, "train_tcnn"

    def __init__(self, state_dict=None, seed=0, lr=1e-3, device="cuda:0", betas=(0.9, 0.999), eps=1e-8):
        sd = tcnn_default_state_dict(seed) if state_dict is None else {k: _np(v) for k, v in state_dict.items()}
        _require(sd, TCNN_KEYS, TCNN_SHAPES)
        super().__init__(sd, seed, lr, device, betas, eps)
        self.adam_step = torch.zeros(1, dtype=torch.int64, device=self.device)   # advanced on the device

    def step(self, input_pts, training_pts, gt, n=None):
        """One training step on a batch: input_pts [B, 64, 6], training_pts [B, M, 3], gt [B, M].  The first ``n``
        points of every patch feed the encoder (None: drawn).  Returns device tensors {"loss", "bce_loss",
        "reg_loss", "skipped"} (skipped: bool, the step left the weights and Adam's state as they were); nothing
        synchronises."""
        n = self.draw_n() if n is None else int(n)
        x, p, g, B, M, ws = self._inputs(input_pts, training_pts, gt, n)
        loss = torch.empty(4, dtype=torch.float32, device=self.device)
        self._call("step", self.params, self.grads, self.exp_avg, self.exp_avg_sq, self.adam_step, x, p, g, B, n, M,
                   *self._adam_args(), loss, ws, ws.numel())
        return {"loss": loss[0], "bce_loss": loss[1], "reg_loss": loss[2], "skipped": loss[3] != 0}

    def eval_loss(self, batch, n=N_LOCAL_SAMPLES):
        """Validation loss: all 64 points; returns the L1 term as a device scalar.  ``batch``: a dict with input_pts,
        training_pts, gt."""
        x, p, g, B, M, ws = self._inputs(batch["input_pts"], batch["training_pts"], batch["gt"], n)
        loss = torch.empty(3, dtype=torch.float32, device=self.device)
        self._call("eval_loss", self.params, x, p, g, B, n, M, loss, ws, ws.numel())
        return loss[1]

    def forward(self, input_pts, training_pts, n=N_LOCAL_SAMPLES):
        """feats [B, 8] and pred [B, M] of the current weights (device tensors, f16 values)."""
        x, p, _, B, M, ws = self._inputs(input_pts, training_pts, torch.zeros(np.shape(training_pts)[:2]), n)
        feats = torch.empty(B, 8, dtype=torch.float32, device=self.device)
        pred = torch.empty(B, M, dtype=torch.float32, device=self.device)
        self._call("forward", self.params, x, p, B, n, M, feats, pred, ws, ws.numel())
        return feats, pred

    def state_dict(self):
        """The weights as numpy arrays with exactly the keys, shapes and dtypes of weights/pointnet_tcnn.npz."""
        return {k: v.copy() for k, v in _views(self.params.cpu().numpy(), TCNN_SHAPES).items()}

    def save_ckpt(self, path):
        """Writes ``{"state_dict": {the two flat vectors}}``, what the reference's LitFusionPointNet(tiny_cuda=True)
        loads strictly (its pretrained/pointnet_tcnn.ckpt holds exactly these keys)."""
        torch.save({"state_dict": {k: torch.from_numpy(v) for k, v in self.state_dict().items()}}, path)

    def to_model(self, voxel_size=0.01, min_pts_in_grid=MIN_PTS_IN_GRID, device=None):
        """A frozen tiny-cuda-nn LitFusionPointNet with these weights, repacked for the inference kernels."""
        from .fusion import load_pretrained
        return load_pretrained(device=device or self.device, voxel_size=voxel_size, min_pts_in_grid=min_pts_in_grid,
                               tiny_cuda=True, state_dict=self.state_dict())
