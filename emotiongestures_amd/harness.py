"""Evaluation harness of the audio->gesture path.

Mirrors what the reference's eval loop does around the generator
(test_emotion_gesture_diversity_iterative.py:191-261): CVAE sample -> generator -> pose, then the FGD auto-encoder
features of predicted and target poses (model/FGD.py:26-82), their Frechet distance and diversity score
(model/FHD_score.py:159-217,247-311), MPJRE, pose L2 and the emotion accuracy of a skeleton classifier
(skeleton_classifer/Models.py:199-283).  The beat-alignment score (model/Beat_score_v2.py, :241-248) is opt-in (``evaluate(...,
beat=True)``): it runs batched on the GPU through :mod:`emotiongestures_amd.beat`, whose audio half is restated from librosa 0.10's
documented onset routines and is not pinned against librosa itself.

Every network forward runs on the GPU through libemogest_hip.so (the FGD encoder and the classifier are built from the
same Linear / attention / LayerNorm operators as the generator); the Gaussian statistics and the matrix square root
stay float64 numpy/scipy on the host exactly as upstream.
"""
from __future__ import annotations

from typing import Dict, Iterable, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from . import ops
from ._host import int_list, stream
from .modules import Encoder, Linear, ReplicaAware, _eval_only, _seq, replica_forward
from .takes import take_distance, take_diversity, track_features  # noqa: F401  (re-exported: the whole-track FGD features / take diversity)

__all__ = ["MLP_Reconstruct", "SkeletonTransformer", "Prior_Encoder", "compute_acc", "l2_distance_pose", "mpjre", "calc_motion",
           "calculate_frechet_distance", "calculate_diversity", "diversity_score", "evaluate", "track_features", "take_distance",
           "take_diversity", "synthesize_takes"]


class _PackCache:
    """Packed (EG_PACK_LINEAR) copies of nn.Linear weights, rebuilt only when the parameter changes."""

    def __init__(self):
        self._c: Dict[int, tuple] = {}

    def get(self, lin: Linear, device, pad_k: int = 0):
        """pad_k > 0: the weight gets that many zero columns first (K not a multiple of 4, e.g. pose_dim 126 / 282)."""
        key = id(lin)
        ver = (lin.weight._version, str(device), pad_k)
        hit = self._c.get(key)
        if hit is None or hit[0] != ver:
            w = lin.weight if not pad_k else torch.cat([lin.weight, lin.weight.new_zeros(lin.weight.shape[0], pad_k)], 1)
            hit = (ver, ops.pack_linear_weight(w, device), w.detach())
            self._c[key] = hit
        return hit[1]

    def padded_weight(self, lin: Linear):
        return self._c[id(lin)][2]


def _affine_chain(cache: _PackCache, x: torch.Tensor, layers, relu_between: bool, precision: str) -> torch.Tensor:
    """x [rows, K] through Linear layers (optionally ReLU between them, never after the last)."""
    for i, lin in enumerate(layers):
        last = i == len(layers) - 1
        k = lin.weight.shape[1]
        if k % 4:                         # e.g. pose_dim 282/126: pad K with zero columns (layout plumbing)
            pad = (-k) % 4
            x = torch.cat([x, x.new_zeros(x.shape[0], pad)], 1)
            packed = cache.get(lin, x.device, pad_k=pad)
            x = ops.linear(x, cache.padded_weight(lin), lin.bias, relu=relu_between and not last, precision=precision, packed=packed)
        elif x.shape[0] <= 64 and k >= 8192:
            x = ops.linear_splitk(x, lin.weight, lin.bias, relu=relu_between and not last, splits=max(1, k // 512), precision=precision,
                                  packed=cache.get(lin, x.device))
        else:
            x = ops.linear(x, lin.weight, lin.bias, relu=relu_between and not last, precision=precision, packed=cache.get(lin, x.device))
    return x


class MLP_Reconstruct(ReplicaAware, nn.Module):
    """model/FGD.py:26-82: per-frame pose auto-encoder whose 512-d latent is the FGD feature.  ``pose_dim`` is 282 upstream
    (hard-coded :32,58); Dropout layers are identity in eval."""

    def __init__(self, bath=True, *, pose_dim=282, precision="f32"):
        super().__init__()
        self.Encoder = _seq(Linear(pose_dim, 512), None, Linear(512, 512), None, Linear(512, 512))
        self.Decoder = _seq(Linear(512, 512), None, Linear(512, 512), None, Linear(512, pose_dim))
        self.precision = precision
        self._cache = _PackCache()

    @replica_forward
    def forward(self, Input):
        _eval_only(self)
        shp = Input.shape
        x = Input.reshape(-1, shp[-1]).contiguous()
        latent = _affine_chain(self._cache, x, [self.Encoder[0], self.Encoder[2], self.Encoder[4]], False, self.precision)
        out = _affine_chain(self._cache, latent, [self.Decoder[0], self.Decoder[2], self.Decoder[4]], False, self.precision)
        return out.view(*shp[:-1], out.shape[-1]), latent.view(*shp[:-1], 512)


class Prior_Encoder(nn.Module):
    """skeleton_classifer/Models.py:88-116"""

    def __init__(self, pose_dim, d_model):
        super().__init__()
        self.fc1, self.fc2 = Linear(pose_dim, d_model), Linear(d_model, d_model)


class SkeletonTransformer(ReplicaAware, nn.Module):
    """skeleton_classifer/Models.py:199-283: emotion classifier on a pose sequence -> (logits [B,8], mid_feature [B,T,d])."""

    def __init__(self, class_dim=8, pose_dim=242, src_pad_idx=1, trg_pad_idx=1, d_word_vec=64, d_model=64, d_inner=512,
                 n_layers=3, n_head=8, d_k=32, d_v=32, dropout=0.2, n_position=60, *, precision="f32"):
        super().__init__()
        assert d_model == d_word_vec
        self.d_model = d_model
        self.prior_seq_encoder = Prior_Encoder(pose_dim, d_model)
        self.post_projector = _seq(Linear(n_position * d_model, d_model * 4), None, Linear(d_model * 4, d_model), None,
                                   Linear(d_model, 128), None, Linear(128, 64), None, Linear(64, class_dim))
        self.encoder = Encoder(n_position=n_position, d_word_vec=d_word_vec, d_model=d_model, d_inner=d_inner, n_layers=n_layers,
                               n_head=n_head, d_k=d_k, d_v=d_v, pad_idx=src_pad_idx, dropout=dropout)
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)
        self.precision = precision
        self._cache = _PackCache()

    @replica_forward
    def forward(self, prior_seq):
        _eval_only(self)
        B, T, D = prior_seq.shape
        for layer in self.encoder.layer_stack:
            layer.slf_attn.precision = layer.pos_ffn.precision = self.precision
        x = _affine_chain(self._cache, prior_seq.reshape(B * T, D).contiguous(), [self.prior_seq_encoder.fc1, self.prior_seq_encoder.fc2],
                          False, self.precision).view(B, T, self.d_model)
        enc, *_ = self.encoder(x, None)
        mid = enc
        head = [self.post_projector[i] for i in (0, 2, 4, 6, 8)]
        logits = _affine_chain(self._cache, enc.reshape(B, -1).contiguous(), head, True, self.precision)
        return logits, mid


# ---- training-side types on the path, forward only ---------------------------------------------------
class Motion_Discriminator(ReplicaAware, nn.Module):
    """Full_model/Models_spatial_memory.py:620-669 (identical class in Models_memory.py): encoder over the motion offsets,
    per-frame Linear+ReLU, 6-layer ReLU MLP -> [B, 1] logit (no sigmoid).  Its forward needs pose_dim == d_word_vec == d_model
    (the encoder adds a d_word_vec-wide table to the raw offsets and fc1 consumes the d_model-wide encoder output as if it were
    pose_dim wide), which the upstream defaults (128 vs 282) violate; the constructor refuses such a combination up front.
    eval(): the inference kernels; train(): the differentiable operators of emotiongestures_amd/train (gradient goldens from the reference:
    tests/golden/adv_grads.npz)."""

    def __init__(self, frames=59, pose_dim=282, src_pad_idx=1, trg_pad_idx=1, d_word_vec=128, d_model=128, d_inner=1024, n_layers=2,
                 n_head=8, d_k=64, d_v=64, dropout=0.2, n_position=59, *, precision="f32"):
        super().__init__()
        if not (pose_dim == d_word_vec == d_model):
            raise ValueError(f"Motion_Discriminator: forward needs pose_dim == d_word_vec == d_model (got {pose_dim}, {d_word_vec}, "
                             f"{d_model}); the upstream defaults fail at the first tensor add")
        self.d_model, self.frames = d_model, frames
        self.encoder = Encoder(n_position=n_position, d_word_vec=d_word_vec, d_model=d_model, d_inner=d_inner, n_layers=n_layers,
                               n_head=n_head, d_k=d_k, d_v=d_v, pad_idx=src_pad_idx, dropout=dropout)
        self.fc1 = _seq(Linear(pose_dim, 64), None)
        self.fc2 = _seq(Linear(frames * 64, 2048), None, Linear(2048, 1024), None, Linear(1024, 256), None, Linear(256, 64), None,
                        Linear(64, 16), None, Linear(16, 1))
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)
        self.precision = precision
        self._cache = _PackCache()

    @replica_forward
    def forward(self, x):
        B, T, D = x.shape
        if T != self.frames or D != self.d_model:
            raise ValueError(f"Motion_Discriminator.forward: expected [B, {self.frames}, {self.d_model}], got {tuple(x.shape)}")
        if self.training:           # train() mode: differentiable HIP operators (emotiongestures_amd/train), gradients for its parameters and for x
            from .train import nets
            return nets.motion_discriminator_forward(self, x)
        for layer in self.encoder.layer_stack:
            layer.slf_attn.precision = layer.pos_ffn.precision = self.precision
        enc, *_ = self.encoder(x.contiguous(), None)
        h = ops.linear(enc.reshape(B * T, D).contiguous(), self.fc1[0].weight, self.fc1[0].bias, relu=True, precision=self.precision,
                       packed=self._cache.get(self.fc1[0], x.device))
        head = [self.fc2[i] for i in (0, 2, 4, 6, 8, 10)]
        return _affine_chain(self._cache, h.reshape(B, -1).contiguous(), head, True, self.precision)


class Pose_Discriminator(ReplicaAware, nn.Module):
    """Full_model/Models_spatial_memory.py:671-704: encoder over a pose sequence -> per-frame Linear(282, 64) -> Dropout(0.2) -> Linear(64, 1)
    -> sigmoid: one real / fake probability per frame, [B, T, 1].  The head is hard-coded to 282 inputs and consumes the d_model-wide encoder
    output directly, and the encoder adds a d_word_vec-wide positional table to the raw poses: the forward is consistent only for
    d_word_vec == d_model == pose_dim (282 upstream), which the upstream defaults (128) violate -- refused up front, as Motion_Discriminator.
    `pose_dim` is a keyword of this build (upstream: the literal 282).  eval(): the inference kernels; train(): the differentiable operators
    (train/nets.pose_discriminator_forward), the 0.2 Dropout active with `train_dropout`."""

    def __init__(self, src_pad_idx=1, trg_pad_idx=1, d_word_vec=128, d_model=128, d_inner=1024, n_layers=3, n_head=8, d_k=64, d_v=64,
                 dropout=0.2, n_position=60, *, pose_dim=282, precision="f32"):
        super().__init__()
        if not (pose_dim == d_word_vec == d_model):
            raise ValueError(f"Pose_Discriminator: forward needs d_word_vec == d_model == {pose_dim} (got {d_word_vec}, {d_model}); "
                             "the upstream defaults fail at the first tensor add")
        self.d_model = d_model
        self.encoder = Encoder(n_position=n_position, d_word_vec=d_word_vec, d_model=d_model, d_inner=d_inner, n_layers=n_layers,
                               n_head=n_head, d_k=d_k, d_v=d_v, pad_idx=src_pad_idx, dropout=dropout)
        self.fc = _seq(Linear(pose_dim, 64), None, Linear(64, 1))
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)
        self.precision = precision

    @replica_forward
    def forward(self, x):
        B, T, D = x.shape
        if D != self.d_model:
            raise ValueError(f"Pose_Discriminator.forward: expected [B, T, {self.d_model}], got {tuple(x.shape)}")
        from .train import functional as TF
        from .train import nets
        if self.training:
            return nets.pose_discriminator_forward(self, x)
        # eval(): the same HIP operators without a tape and with every Dropout off.  (The fused inference blocks -- eg_multi_head_attention,
        # eg_positionwise_ffn -- stream 16-byte-aligned rows; a 282-wide model is not, so the encoder runs operator by operator here.)
        with TF.precision(self.precision if self.precision in ("f32", "bf16x3") else "f32"), torch.no_grad():
            return nets.pose_discriminator_forward(self, x, dropout=False)


class SoftmaxContrastiveLoss(nn.Module):
    """test_emotion_gesture_diversity_iterative.py:80-127 on the GPU (eg_contrastive_loss: one workgroup per row, fixed-order
    reductions).  forward -> scalar loss tensor (differentiable when an input requires a gradient: eg_contrastive_loss_backward);
    evaluate -> (accuracy, cross_dist [n, n])."""

    def _run(self, face_feat, audio_feat, want_cross):
        if face_feat.dim() != 2 or face_feat.shape != audio_feat.shape:
            raise ValueError(f"SoftmaxContrastiveLoss: expected two [n, d] tensors, got {tuple(face_feat.shape)} and {tuple(audio_feat.shape)}")
        if not face_feat.is_cuda or not audio_feat.is_cuda:
            raise RuntimeError("SoftmaxContrastiveLoss runs on the GPU only (no CPU fallback)")
        lib = L.load()
        f, a = face_feat.detach().float().contiguous(), audio_feat.detach().float().contiguous()
        n, d = f.shape
        dev = f.device
        cross = torch.empty(n, n, device=dev) if want_cross else None
        res = torch.empty(2, device=dev)
        nbytes = int(lib.eg_contrastive_workspace_bytes(n))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        p = lambda t: None if t is None else t.data_ptr()
        L.check(lib.eg_contrastive_loss(p(f), p(a), n, d, p(cross), res[0:1].data_ptr(), res[1:2].data_ptr(), p(ws), nbytes,
                                        stream(dev)), "eg_contrastive_loss")
        return res[0], res[1], cross

    @torch.no_grad()
    def evaluate(self, face_feat, audio_feat, mode="max"):
        if mode != "max":
            raise ValueError(mode)
        _loss, acc, cross = self._run(face_feat, audio_feat, True)
        return acc, cross

    def forward(self, face_feat, audio_feat, contrastive_device, mode="max"):
        if mode != "max":
            raise ValueError(mode)
        dev = torch.device(contrastive_device)
        if torch.is_grad_enabled() and (face_feat.requires_grad or audio_feat.requires_grad):
            from .train import functional as TF
            return TF.contrastive_loss(face_feat.to(dev), audio_feat.to(dev)).reshape(())
        return self._run(face_feat.to(dev), audio_feat.to(dev), False)[0]


def adjust_lr(optimizer, init_lr, epoch, decay_rate=0.1, decay_epoch=4):
    """test_emotion_gesture_diversity_iterative.py:64-78: piecewise-constant learning rate written into every param group
    (`decay_rate` / `decay_epoch` are accepted and ignored, as upstream).  Past epoch 150 upstream dies on an unbound local;
    here that is a ValueError."""
    if epoch <= 15:
        lr = init_lr
    elif epoch <= 50:
        lr = init_lr * 0.2
    elif epoch <= 80:
        lr = init_lr * 0.01
    elif epoch <= 100:
        lr = init_lr * 0.005
    elif epoch <= 150:
        lr = init_lr * 0.001
    else:
        raise ValueError(f"adjust_lr: the schedule is defined for epochs 0..150 (got {epoch})")
    for param_group in optimizer.param_groups:
        param_group["lr"] = lr


def set_requires_grad(nets, requires_grad=False):
    """test_emotion_gesture_diversity_iterative.py:51-62"""
    if not isinstance(nets, list):
        nets = [nets]
    for net in nets:
        if net is not None:
            for param in net.parameters():
                param.requires_grad = requires_grad


# ---- metrics (host side, as upstream) ---------------------------------------------------------------------------------
def compute_acc(input_label: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """test_emotion_gesture_diversity_iterative.py:35-39"""
    pred = out.topk(1, 1)[1].squeeze(1)
    return 100 * torch.true_divide(torch.sum(pred == input_label), input_label.size(0))


def calc_motion(motion: torch.Tensor) -> torch.Tensor:
    """test_emotion_gesture_diversity_iterative.py:41-44 (frame-to-frame offsets; 60 upstream = n_frames)."""
    n = motion.shape[1]
    return motion[:, 1:n, :] - motion[:, : n - 1, :]


def l2_distance_pose(fake: np.ndarray, gt: np.ndarray) -> float:
    """test_emotion_gesture_diversity_iterative.py:46-49"""
    return float(np.mean(np.linalg.norm(gt - fake, axis=-1)))


def mpjre(target: torch.Tensor, pred: torch.Tensor) -> float:
    """Mean per-joint rotation error term, :223 (mean |target - pred| over 6-d groups)."""
    b = target.shape[0]
    return float(torch.mean(torch.absolute(target.reshape(b, -1, 6) - pred.reshape(b, -1, 6))))


def calculate_frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6, imaginary="return_100"):
    """model/FHD_score.py:159-217: ||mu1-mu2||^2 + Tr(C1 + C2 - 2 sqrt(C1 C2)), float64, scipy sqrtm.  Any ValueError raised
    inside upstream's try block (a non-negligible imaginary part of the square root, or scipy rejecting the product, e.g. NaN / inf entries) returns
    100 as that file does (`imaginary="return_100"`); model/embedding_space_evaluator.py:156-209 carries the same formula without the try, so
    the ValueError propagates there (`imaginary="raise"`) -- its one difference, so that copy delegates here."""
    from scipy import linalg

    mu1, mu2 = np.atleast_1d(mu1), np.atleast_1d(mu2)
    sigma1, sigma2 = np.atleast_2d(sigma1), np.atleast_2d(sigma2)
    assert mu1.shape == mu2.shape and sigma1.shape == sigma2.shape
    diff = mu1 - mu2
    try:        # upstream's try covers the square root, the singular-product retry and the trace: ANY ValueError in there returns 100 (:196-213)
        covmean, _ = linalg.sqrtm(sigma1.dot(sigma2), disp=False)
        if not np.isfinite(covmean).all():
            offset = np.eye(sigma1.shape[0]) * eps
            covmean = linalg.sqrtm((sigma1 + offset).dot(sigma2 + offset))
        if np.iscomplexobj(covmean):
            if not np.allclose(np.diagonal(covmean).imag, 0, atol=1e-3):
                raise ValueError("Imaginary component {}".format(np.max(np.abs(covmean.imag))))
            covmean = covmean.real
        tr_covmean = np.trace(covmean)
    except ValueError:
        if imaginary == "raise":
            raise
        return 100
    return diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * tr_covmean


class FrechetAccumulator:
    """Running first and second moments of feature rows ON THE DEVICE ("(sum x, sum x x^T) accumulators"):
    the Frechet distance of model/FHD_score.py:159-217 needs only the mean and covariance of the [N, 512] feature rows, so a
    long evaluation (or several ranks) never has to hold or gather the rows themselves.

    push(rows [N, D] on the GPU):  s += colsum(x - c);  S += (x - c)^T (x - c)   (eg_colsum / eg_gemm_tn, fp32, fixed-order sums;
    c = a fixed shift -- the first batch's column mean by default -- keeps S - s s^T / n well conditioned).
    stats() -> (mu, sigma) in float64 on the host, the same estimator as np.mean / np.cov(rowvar=False).
    all_reduce(): sums (n, s, S) over the ranks of a process group (D + D^2 + 1 numbers per rank); every rank
    must use the same shift (pass `shift=` explicitly, e.g. zeros)."""

    def __init__(self, dim: int = 512, device="cuda", shift: Optional[torch.Tensor] = None):
        self.dim, self.device = dim, torch.device(device)
        self.n = 0
        self.s = torch.zeros(dim, device=self.device)
        self.S = torch.zeros(dim, dim, device=self.device)
        self.shift = None if shift is None else shift.to(self.device, torch.float32).contiguous()

    def push(self, rows: torch.Tensor) -> None:
        from .train import functional as TFn
        x = rows.detach().reshape(-1, self.dim)
        if not x.is_cuda:
            raise L.EgError("FrechetAccumulator.push: rows must be on the GPU (no CPU fallback)")
        x = x.float().contiguous()
        if self.shift is None:
            self.shift = TFn.raw_ew(TFn.EW_SCALE, TFn.raw_colsum(x)[0], None, 1.0 / x.shape[0])
        xc = ops.add_rows(x, TFn.raw_ew(TFn.EW_SCALE, self.shift, None, -1.0).view(1, -1), period=1)
        self.s = TFn.raw_ew(TFn.EW_ADD, self.s, TFn.raw_colsum(xc)[0])
        TFn.raw_gemm_tn(xc, xc, out=self.S, accumulate=True)
        self.n += x.shape[0]

    def all_reduce(self, group=None) -> None:
        import torch.distributed as dist
        n = torch.tensor([float(self.n)], device=self.device, dtype=torch.float64)
        for t in (n, self.s, self.S):
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
        self.n = int(round(float(n.item())))

    def stats(self):
        n = self.n
        if n < 2:
            raise ValueError("FrechetAccumulator.stats: need at least two rows")
        s, S = self.s.double().cpu().numpy(), self.S.double().cpu().numpy()
        mu = self.shift.double().cpu().numpy() + s / n
        sigma = (S - np.outer(s, s) / n) / (n - 1)
        return mu, (sigma + sigma.T) / 2


def calculate_diversity(activations: np.ndarray, labels, diversity_times: int = 5) -> np.float32:
    """model/FHD_score.py:270-286: mean L2 distance of `diversity_times` random pairs (np.random.randint twice, in that order)."""
    num = len(labels)
    first = np.random.randint(0, num, diversity_times)
    second = np.random.randint(0, num, diversity_times)
    acc = 0.0
    for i, j in zip(first, second):
        acc += float(np.sqrt(((activations[i] - activations[j]) ** 2).sum()))
    return np.float32(acc / diversity_times)


def diversity_score(activations: np.ndarray, frames: int = 60):
    """model/FHD_score.py:247-268: 10 repeats of calculate_diversity -> centre and 95 % normal interval."""
    from scipy import stats

    act = activations.reshape(-1, frames, 512)
    window = np.empty((10, 1))
    for i in range(10):
        window[i] = calculate_diversity(act, act)
    mean, std = np.mean(window, axis=0), np.std(window, axis=0)
    interval = stats.norm.interval(0.95, mean, std)
    return (interval[0] + interval[1]) / 2, interval


# ---- the eval loop ---------------------------------------------------------------------------------------------------
def evaluate(generator, vae, fgd: MLP_Reconstruct, classifier: Optional[SkeletonTransformer], batches: Iterable[dict],
             n_pre_poses: int, device="cuda", z_list: Optional[list] = None, beat: bool = False, fps: int = 15) -> Dict[str, float]:
    """One pass of test_model's hot loop (:191-261) over an iterable of batches, each a dict with
    ``spec [B,128,T]``, ``text [B,60]``, ``pose_seq [B,F,D]`` (target; the first n_pre_poses frames are the prior) and
    ``label [B,8]`` one-hot.  ``z_list`` optionally fixes the CVAE latents per batch (default: torch.randn on the CPU
    generator as upstream).  Returns the metrics of the summary line (:261); the beat score only with ``beat=True``
    (opt-in, see the module docstring): then every batch also carries ``audio [B, n]`` (16 kHz) and ``"beat"`` is the mean per-clip
    score of the predicted poses (t_start 0, t_end int(F / fps), sigma 0.3, order 2: BL_score / (len(loader) * batch) for full
    batches).  A clip without audio onsets raises ValueError (upstream dies there with ZeroDivisionError)."""
    pred_feats, tgt_feats, l2s, rots, accs, beats = [], [], [], [], [], []
    frames = None
    with torch.no_grad():
        for bi, batch in enumerate(batches):
            pose_seq = batch["pose_seq"].to(device)
            frames = pose_seq.shape[1]
            pre_pose = pose_seq[:, :n_pre_poses].contiguous()
            label = batch["label"].to(device)
            sampled = vae.sample(label, z=None if z_list is None else z_list[bi])                                    # :203
            pred_pose, _, _, _, _ = generator(batch["spec"].to(device), batch["text"].to(device), pre_pose, sampled)  # :205
            if classifier is not None:
                logits, _ = classifier(pred_pose)                                                                    # :217
                accs.append(float(compute_acc(torch.max(label, 1)[1], logits)))
            rots.append(mpjre(pose_seq, pred_pose))                                                                 # :223
            _, pf = fgd(pred_pose)                                                                                   # :226-229
            _, tf = fgd(pose_seq)
            pred_feats.append(pf.reshape(-1, 512).cpu().numpy().astype(np.float64))
            tgt_feats.append(tf.reshape(-1, 512).cpu().numpy().astype(np.float64))
            l2s.append(l2_distance_pose(pred_pose.cpu().numpy().astype(np.float32), pose_seq.cpu().numpy().astype(np.float32)))
            if beat:                                                                                                 # :241-248
                from .beat import beat_alignment
                sc = beat_alignment(batch["audio"].to(device), pred_pose, fps=fps, t_start=0, t_end=int(frames / fps)).cpu().numpy()
                bad = np.flatnonzero(np.isnan(sc))
                if bad.size:
                    raise ValueError(f"evaluate: batch {bi} clip {int(bad[0])} has no audio onsets (the beat score divides by their count)")
                beats.append(sc)
    pred_arr, tgt_arr = np.concatenate(pred_feats), np.concatenate(tgt_feats)
    fid = calculate_frechet_distance(np.mean(pred_arr, axis=0), np.cov(pred_arr, rowvar=False),
                                     np.mean(tgt_arr, axis=0), np.cov(tgt_arr, rowvar=False))                       # :250-255
    div, interval = diversity_score(pred_arr, frames)                                                               # :256
    out = {"pose_l2": float(np.mean(l2s)), "rotation_deg": float(np.mean(rots)) * 57.2958, "fgd": float(np.real(fid)),
           "diversity": float(np.ravel(div)[0]), "diversity_lo": float(np.ravel(interval[0])[0]), "diversity_hi": float(np.ravel(interval[1])[0])}
    if accs:
        out["emotion_acc"] = float(np.mean(accs))
    if beat:
        out["beat"] = float(np.mean(np.concatenate(beats)))
    return out


# ---- long-form synthesis ---------------------------------------------------------------------------------------------
def synthesize(models, audio: torch.Tensor, text: torch.Tensor, seed_pose: torch.Tensor, labels: Optional[torch.Tensor] = None,
               hop_samples: Optional[int] = None, n_samples: Optional[int] = None, windows: Optional[int] = None,
               z: Optional[torch.Tensor] = None, alpha: Optional[torch.Tensor] = None, fps: int = 15, sample_rate: int = 16000,
               want_windows: bool = False, want_aux: bool = False, mel=None, lengths=None, draws: Optional[int] = None,
               beat: bool = False, diversity=None, audio_rate: Optional[int] = None, joints=None, joints_mean=None,
               joints_unit: bool = False, joints_fps=None, rotations=None, rotations_space: str = "local", smooth=None, euler=None,
               euler_unwrap: bool = False, kinematics=None, srgr=None, l1div: bool = False, emotion=None,
               emotion_stride: Optional[int] = None, diversity_stride: int = 34, bvh_text: bool = False, preview=None) -> Dict[str, torch.Tensor]:
    """One gesture track per utterance from raw 16 kHz audio: windows -> mel -> optional CVAE sample per window -> roll-out.

    ``models = (generator, vae | None)``, eval mode, on the GPU.  ``audio [U, total_samples]``; ``text [U, W, 60]`` (the words of every
    window); ``seed_pose [U, prior_frames, pose_dim]``; ``labels`` (with a VAE) ``[U, 8]`` or ``[U, W, 8]`` one-hot, ``z [U, W, 32]``
    fixes the latents (default torch.randn on the CPU generator, as MLP_Reconstruct_v3.sample draws them).  Window w covers samples
    ``[w*hop_samples, w*hop_samples + n_samples)``; the defaults tie them to the generator's geometry: ``hop_samples`` is the duration of
    ``frames - prior_frames`` poses at ``fps``, ``n_samples = (spec_len - 1) * 512`` (the shortest clip whose spectrogram has spec_len
    columns).  ``windows`` defaults to ``text.shape[1]``.  Returns GeneratorEngine.forward_rollout's dict plus ``"spec"``.

    ``lengths`` (U sample counts): recordings of unequal length, ``audio [U, max_total]`` with ``lengths[u]`` real samples in row u (the rest
    is never read).  Recording u then has ``W_u = ceil(lengths[u] / hop_samples)`` windows -- every window that starts inside it, the count a
    stream reaches for a row ended at that length; ``text``, ``labels`` and ``z`` are per recording (labels ``[U, 8]`` only), padded
    ``[U, max W_u, ...]`` or packed ``[sum W_u, ...]``; ``windows`` is not used.  Returns GeneratorEngine.forward_rollout_ragged's dict plus
    packed ``"spec"`` and ``"windows_per"``.

    ``draws=R`` (a VAE is required): R sampled tracks per recording in one call.  ``z [U, R, W, 32]`` (default torch.randn on the CPU generator
    in that shape), ``labels`` ``[U, 8]``, ``[U, W, 8]`` or ``[U, R, W, 8]`` (each draw its own emotion); one ``vae.sample`` at batch
    ``U*R*W``, mel and window gather once per recording.  Returns GeneratorEngine.forward_rollout_draws's dict (track ``[U, R, T, pose_dim]``)
    plus ``"spec"``.  Rectangular calls only: not with ``lengths`` -- recordings of unequal length with draws are ``synthesize_takes``.

    ``beat=True`` (opt-in; BEAT-shaped generators, pose_dim >= 174): adds ``"beat"``, the beat-alignment score of every returned track
    against the audio it was made from (beat.beat_alignment_tracks: fp64 ``[U]``, or ``[U, R]`` with ``draws``), recording u scored on its
    own ``lengths[u]`` samples and its own ``W_u * (frames - prior_frames) + prior_frames`` poses.

    ``diversity=fgd`` (an eval-mode ``MLP_Reconstruct``; with ``draws=R``, R >= 2): adds ``"take_distance"`` ``[U, R, R]`` and
    ``"take_diversity"`` ``[U]`` (fp64), the pairwise distances of the returned takes of every recording in FGD feature space and their mean
    (takes.take_diversity with ``span = frames``: the unit of the clip metric ``calculate_diversity`` on one generator window).
    ``diversity=ae`` (an eval-mode ``model.motion_ae.MotionAE`` whose ``pose_dim`` is the generator's: the TED-Expressive feature space): the
    same two keys from ``motionfeat.window_features`` -- the encoder on every 34-frame window of every take at stride ``diversity_stride``
    (default 34), one fused launch for the convolutions -- with ``span = 1``: the RMS per-window feature distance, comparable across
    recording lengths.  A net of another pose width, in train mode, or a generator whose shortest track has fewer than 34 poses is refused
    by name before anything runs.

    ``audio_rate`` (Hz; e.g. 48000, 44100, 24000): ``audio``, and ``lengths`` when given, are at that rate.  The audio is resampled to
    ``sample_rate`` once on the device (resample.resample_audio: scipy's ``resample_poly`` design, ``max(L, M) <= 640``), then the path above
    runs unchanged on the result -- with ``lengths``, ``draws``, ``beat`` (scored against the resampled audio and its lengths) and
    ``diversity``; ``hop_samples`` / ``n_samples`` stay in model-rate samples.  The dict gains ``"audio"`` (the resampled signal) and, with
    ``lengths``, ``"lengths"`` (its sample counts).  ``None`` or equal to ``sample_rate``: no launch and no extra keys.

    ``joints=skeleton`` (a ``skeleton.Skeleton`` with ``3K == pose_dim``, e.g. ``skeleton.ted_expressive()``): adds ``"joints"``, the joint
    positions of every returned track in metres -- ``[U, T', J, 3]``, or ``[U, R, T', J, 3]`` with ``draws`` -- and ``"joint_frames"`` (U ints):
    ``skeleton.joints_from_tracks(out["track"], skeleton, frames, joints_mean, joints_unit, joints_fps)`` with recording u's own
    ``W_u * (frames - prior_frames) + prior_frames`` valid poses, one launch.  ``joints_mean [pose_dim]``: the data set's mean direction vectors,
    added first; ``joints_unit``: bones re-normalised to unit length; ``joints_fps=(src, dst)``: resampled linearly to the renderer's rate
    (``T' = ceil(T * dst / src)``).  Works with ``lengths``, ``draws``, ``beat``, ``diversity`` and ``audio_rate``; without ``joints`` nothing
    changes.

    ``rotations=rest`` (with ``joints=skeleton``; ``rest [K, 3]``, the direction of every bone in the avatar's bind pose): adds ``"rotations"``,
    one unit quaternion ``(w, x, y, z)`` per bone and output frame -- ``[U, T', K, 4]``, or ``[U, R, T', K, 4]`` with ``draws`` -- relative to
    the parent bone (``rotations_space="local"``, what a rig takes) or to the root (``"global"``):
    ``skeleton.rotations_from_tracks(out["track"], skeleton, rest, frames, joints_mean, joints_fps, rotations_space)``, one more launch, on the
    frames ``"joint_frames"`` counts.

    ``joints=tree`` (a ``skeleton.JointTree`` with ``6J == pose_dim``: the BEAT generators, whose columns are 6-D joint rotations):
    ``"joints"`` ``[U, (R,) T', J, 3]`` and ``"joint_frames"`` as above, and with ``rotations=True`` ``"rotations"`` ``[U, (R,) T', J, 4]`` in
    ``rotations_space`` -- ``skeleton.joints_from_rot6d`` / ``rotations_from_rot6d`` of the track, both from ONE launch
    (``skeleton.launch_articulate``).  ``joints_mean [6J]`` and ``joints_fps`` as above; ``joints_unit`` and a rest pose are refused by name
    (the tree's offsets are the bind pose).  With ``smooth=`` the filtered 6-D rows are re-orthonormalised by Gram-Schmidt on the way to the
    matrices: this is the sanctioned way to smooth rotations (there is no filter over quaternions).

    ``euler=order | BvhFile`` (with ``joints=tree``): adds ``"euler"`` ``[U, (R,) T', J, 3]``, the BVH rotation channels of every joint in
    degrees on the frames ``"joint_frames"`` counts: ``skeleton.euler_from_rot6d(track, tree, order, frames, joints_mean, joints_fps,
    unwrap=euler_unwrap)``, one more launch (three more with ``euler_unwrap=True``, the Euler filter).  ``order``: one of XYZ .. ZYX for all
    joints, or J of them; a ``bvh.BvhFile`` gives the orders of the tree's joints by name, and its ``format`` / ``write`` then turn one take
    of ``out["euler"]`` into a ``.bvh`` text.  Made from ``"track_smooth"`` with ``smooth=``.  Refused by name: ``euler=`` without
    ``joints=``, and with a ``Skeleton`` (direction-vector bodies have no joint rotations).

    ``bvh_text=True`` (with ``euler=BvhFile``): adds ``"bvh"``, a ``bvh.BvhText``: ``euler.format_tracks(out["euler"], out["joint_frames"],
    tree.names, frame_time=1 / rate)`` at the output rate (``joints_fps[1]`` when given, else ``fps``) -- the ``MOTION`` lines of every take
    formatted on the device, four launches and one small copy of the sizes to the host; ``out["bvh"].text(u, r)`` is ``euler.format`` of that
    take and ``out["bvh"].write(dir)`` writes one ``.bvh`` per take from one copy of the text.  Refused by name before anything runs:
    ``bvh_text=True`` without ``euler=`` being a ``BvhFile``.

    ``preview=PreviewSpec | dict`` (``preview.PreviewSpec``; with ``joints=``): adds ``"preview"``, stick-figure pictures of every frame of
    every take, ``uint8 [U, (R,) T', H, W, 3]`` (or ``[..., 3, H, W]`` with ``layout="chw"``): ``preview.render_joints(out["joints"], spec,
    out["joint_frames"])``, one launch -- of the smoothed joints with ``smooth=`` and at the output rate with ``joints_fps=``, because that is
    what ``out["joints"]`` holds; all-zero bytes behind a recording's frames.  ``preview.write_y4m`` turns one take into a video stream.
    Refused by name before anything runs: ``preview=`` without ``joints=``, a spec whose body is not the ``joints=`` body, and an output
    larger than ``spec.max_bytes``.  Without ``preview`` no key and no launch changes.

    ``smooth=Smoother | (window, polyorder)`` (``smooth.Smoother``; a pair is a filter at ``fps``): adds ``"track_smooth"``, the shape of
    ``"track"``: ``smooth.smooth_tracks(out["track"], smooth, frames)``, a Savitzky-Golay filter (``scipy.signal.savgol_filter``,
    ``mode="interp"``) over recording u's own valid poses, zeros behind them, one launch.  ``"track"`` stays raw and ``beat`` / ``diversity`` keep
    scoring it (they measure the model); ``"joints"`` and ``"rotations"`` are then made from ``"track_smooth"`` (they are what a renderer
    takes).  ``deriv != 0`` is refused by name: a velocity track is not a pose track -- call ``smooth_tracks`` for derivatives.

    ``kinematics=True | edges | SpeedBins`` (with ``joints=``; without it, refused by name): adds ``"kinematics"``, the motion statistics of
    ``out["joints"]`` over the frames ``"joint_frames"`` counts -- ``kinematics.kinematics_of_joints(out["joints"], rate, out["joint_frames"],
    edges)``: ``"speed"``, ``"accel"``, ``"jerk"`` ``[U, (R,) J]`` float64 (the means per joint in m/s, m/s^2, m/s^3), ``"speed_hist"``
    ``[U, (R,) J, B]`` and ``"speed_over"`` ``[U, (R,) J]`` int32 and ``"edges"`` (m/s; ``True``: 0, 0.05 .. 2.0), one read of the joints on the
    device.  ``rate`` is the output rate: ``joints_fps[1]`` when given, else ``fps``.  With ``smooth=`` the figures describe the smoothed
    joints, because that is what ``out["joints"]`` holds; the raw figure is
    ``kinematics_of_joints(skeleton.joints_from_tracks(out["track"], skeleton, frames, joints_mean, joints_unit, joints_fps)[0], rate,
    out["joint_frames"])``.  Works with ``lengths`` and ``draws``; without ``kinematics`` no key and no launch changes.

    ``srgr=SemanticTargets(joints, semantic, threshold)`` (``jointscore.SemanticTargets``; with ``joints=``, without it refused by name): the
    target joints ``[U, T', J, 3]`` and semantic weights ``[U, T']`` of the recordings at the output rate, made from the captured tracks by
    ``skeleton.joints_from_tracks`` / ``joints_from_rot6d`` with this call's ``joints_mean`` / ``joints_unit`` / ``joints_fps``.  Adds
    ``"srgr"``: ``jointscore.srgr_of_joints(out["joints"], targets, semantic, out["joint_frames"], threshold)`` -- ``"srgr"``, ``"recall"``
    ``[U, (R,)]`` float64, ``"hits"`` ``[U, (R,) J]`` int32, ``"frames"`` --, two launches; with ``draws`` the R takes of a recording share its
    target.  Targets whose U, T' or J do not fit are refused by name before anything runs (T' once the generator's geometry is known).
    ``l1div=True`` (with ``joints=``): adds ``"l1div"``, ``jointscore.l1div_of_tracks(out["joints"].flatten(-2), out["joint_frames"])`` --
    ``"l1div"``, ``"l1_sum"`` ``[U, (R,)]`` and ``"mean"`` ``[U, (R,) 3J]`` float64, in metres --, four launches.  Both describe the smoothed
    joints with ``smooth=`` and work with ``lengths`` and ``draws``; without them no key and no launch changes.

    ``emotion=classifier`` (an eval-mode ``SkeletonTransformer`` whose ``pose_dim`` is the generator's; ``emotion_stride``: the stride of its
    windows, default its ``n_position``): adds ``"emotion"``, ``emotion.emotion_of_tracks(classifier, out["track"], frames, labels,
    emotion_stride)`` with recording u's own valid poses -- which emotion the classifier recognises in every take (``"pred"``, ``"votes"``,
    ``"mean_logit"`` ``[U, R, ...]``, R = 1 without ``draws``) and, with a VAE and ``labels``, how often it is the one the take was asked for
    (``"hit"``, ``"accuracy"``, ``"confusion"``, ...).  The raw track is scored, also with ``smooth=``: it measures the model.  The labels
    are the call's own, one per take: ``[U, 8]``, or ``[U, W, 8]`` / ``[U, R, W, 8]`` / the packed forms when constant along a take's
    windows.  Labels that change along a take are refused by name before anything runs (one label per take is what is scored; the pieces
    can be scored with ``emotion_of_tracks``), and so are a classifier of another ``pose_dim`` or in train mode.  Works with ``lengths``,
    ``draws`` and ``audio_rate``; without ``emotion`` no key and no launch changes."""
    outputs = _track_outputs("synthesize", seed_pose, joints, joints_mean, joints_unit, joints_fps, rotations, rotations_space, euler, euler_unwrap)
    kinematics = _kinematics_arg("synthesize", kinematics, outputs, joints_fps, fps)
    srgr, l1div = _jointscore_args("synthesize", srgr, l1div, outputs, audio)
    bvh_text = _bvh_text_arg("synthesize", bvh_text, euler, joints, joints_fps, fps)
    preview = _preview_arg("synthesize", preview, outputs)
    return _synthesize("synthesize", models, audio, text, seed_pose, labels, hop_samples, n_samples, windows, z, alpha, fps, sample_rate,
                       want_windows, want_aux, mel, lengths, draws, beat, diversity, audio_rate, outputs, smooth, takes=False, kinematics=kinematics,
                       srgr=srgr, l1div=l1div, emotion=emotion, emotion_stride=emotion_stride, diversity_stride=diversity_stride,
                       bvh_text=bvh_text, preview=preview)


def synthesize_takes(models, audio: torch.Tensor, text: torch.Tensor, seed_pose: torch.Tensor, labels: Optional[torch.Tensor] = None, *,
                     lengths=None, draws: int, z: Optional[torch.Tensor] = None, alpha: Optional[torch.Tensor] = None,
                     hop_samples: Optional[int] = None, n_samples: Optional[int] = None, fps: int = 15, sample_rate: int = 16000,
                     want_windows: bool = False, want_aux: bool = False, mel=None, beat: bool = False, diversity=None,
                     audio_rate: Optional[int] = None, joints=None, joints_mean=None, joints_unit: bool = False, joints_fps=None,
                     rotations=None, rotations_space: str = "local", smooth=None, euler=None,
                     euler_unwrap: bool = False, kinematics=None, srgr=None, l1div: bool = False, emotion=None,
                     emotion_stride: Optional[int] = None, diversity_stride: int = 34, bvh_text: bool = False, preview=None) -> Dict[str, torch.Tensor]:
    """``draws`` = R sampled takes for each of U recordings of any and unequal length, from raw audio, in one call: ``synthesize(lengths=)`` and
    ``synthesize(draws=)`` combined (a VAE is required).  ``audio [U, max_total]`` with ``lengths[u]`` real samples in row u (``None``: every
    row at full length); recording u has ``W_u = ceil(lengths[u] / hop_samples)`` windows, N = sum W_u.  ``text`` padded ``[U, Wmax, 60]`` or
    packed ``[N, 60]``; ``labels`` ``[U, 8]``, ``[U, Wmax, 8]``, ``[U, R, Wmax, 8]`` (each draw its own emotion) or packed ``[N*R, 8]``;
    ``z [U, R, Wmax, 32]`` or packed ``[N*R, 32]`` (default ``torch.randn(N*R, 32)`` on the CPU generator).  Packed per-take rows are in the
    order of GeneratorEngine.forward_rollout_takes: window w of draw r of recording u at row ``R*off[u] + r*W_u + w``.  Mel and the window
    gather run once per recording, one ``vae.sample`` at batch ``N*R``.  Returns forward_rollout_takes's dict (track ``[U, R, T, pose_dim]``
    zero past ``track_frames[u]``) plus packed ``"spec"`` and ``"windows_per"``.  Every other option is ``synthesize``'s, applied per take with
    recording u's own samples and poses: ``beat`` -> ``"beat"`` ``[U, R]``; ``diversity`` (R >= 2) -> ``"take_distance"`` ``[U, R, R]`` and
    ``"take_diversity"`` ``[U]``; ``joints`` -> ``[U, R, T', J, 3]``; ``rotations`` -> ``[U, R, T', K, 4]``; ``audio_rate``; ``smooth`` ->
    ``"track_smooth"`` ``[U, R, T, pose_dim]``; ``kinematics`` (with ``joints``) -> ``"kinematics"``, the figures ``[U, R, J]`` per take; ``srgr``
    and ``l1div`` (with ``joints``) -> ``"srgr"`` and ``"l1div"``, the figures ``[U, R]`` per take (the takes of a recording share its target);
    ``emotion`` -> ``"emotion"``, the recognised emotion of every take against the label it was asked for (``[U, R]`` per take)."""
    outputs = _track_outputs("synthesize_takes", seed_pose, joints, joints_mean, joints_unit, joints_fps, rotations, rotations_space, euler, euler_unwrap)
    kinematics = _kinematics_arg("synthesize_takes", kinematics, outputs, joints_fps, fps)
    srgr, l1div = _jointscore_args("synthesize_takes", srgr, l1div, outputs, audio)
    bvh_text = _bvh_text_arg("synthesize_takes", bvh_text, euler, joints, joints_fps, fps)
    preview = _preview_arg("synthesize_takes", preview, outputs)
    return _synthesize("synthesize_takes", models, audio, text, seed_pose, labels, hop_samples, n_samples, None, z, alpha, fps, sample_rate,
                       want_windows, want_aux, mel, lengths, draws, beat, diversity, audio_rate, outputs, smooth, takes=True, kinematics=kinematics,
                       srgr=srgr, l1div=l1div, emotion=emotion, emotion_stride=emotion_stride, diversity_stride=diversity_stride,
                       bvh_text=bvh_text, preview=preview)


def _bvh_text_arg(who, bvh_text, euler, joints, joints_fps, fps):
    """The ``bvh_text=`` argument of `synthesize` / `synthesize_takes`, checked before anything runs: (the BvhFile, seconds per output frame), or None."""
    if not bvh_text:
        return None
    if not callable(getattr(euler, "format_tracks", None)):
        raise L.EgError(f"{who}: bvh_text=True needs euler=BvhFile (the text is that file's HIERARCHY and channel layout), got euler="
                        f"{type(euler).__name__}")
    return euler, 1.0 / float(fps if joints_fps is None else joints_fps[1])


def _preview_arg(who, preview, outputs):
    """The ``preview=`` argument of `synthesize` / `synthesize_takes`, checked before anything runs: the PreviewSpec, whose body is the
    ``joints=`` body, or None."""
    if preview is None:
        return None
    if outputs is None:
        raise L.EgError(f"{who}: preview= without joints= (the pictures are those of out[\"joints\"], in metres)")
    from .preview import PreviewSpec
    spec = PreviewSpec.of(preview, f"{who}: preview")
    if spec.body is not outputs.body and spec.body != outputs.body:
        raise L.EgError(f"{who}: preview=: the spec draws {spec.body!r}, joints= is {outputs.body!r}: the bones must name the joints that "
                        "out[\"joints\"] holds")
    spec.check(outputs.body.J)
    return spec


def _kinematics_arg(who, kinematics, outputs, joints_fps, fps):
    """The ``kinematics=`` argument of `synthesize` / `synthesize_takes`, checked before anything runs: the SpeedBins at the output rate, or None."""
    if kinematics is None:
        return None
    if outputs is None:
        raise L.EgError(f"{who}: kinematics= without joints= (the statistics are those of out[\"joints\"], in metres)")
    from . import kinematics as KN
    return KN.SpeedBins.of(kinematics, f"{who}: kinematics", fps if joints_fps is None else joints_fps[1])


def _jointscore_args(who, srgr, l1div, outputs, audio):
    """The ``srgr=`` and ``l1div=`` arguments of `synthesize` / `synthesize_takes`, checked before anything runs: the SemanticTargets (or None)
    against the recordings and the body's joints, and the flag."""
    if srgr is None and not l1div:
        return None, False
    for name, given in (("srgr", srgr is not None), ("l1div", bool(l1div))):
        if given and outputs is None:
            raise L.EgError(f"{who}: {name}= without joints= (the score is that of out[\"joints\"], in metres)")
    if l1div is not True and l1div:
        raise L.EgError(f"{who}: l1div= takes True, got {type(l1div).__name__}")
    if srgr is not None:
        from .jointscore import SemanticTargets
        if not isinstance(srgr, SemanticTargets):
            raise L.EgError(f"{who}: srgr= takes a jointscore.SemanticTargets, got {type(srgr).__name__}")
        srgr.fit(who, U=int(audio.shape[0]) if audio.dim() == 2 else None, J=outputs.body.J)
    return srgr, bool(l1div)


def _motion_ae_arg(who, diversity, stride, gen, seed_pose) -> bool:
    """``diversity=`` as a ``MotionAE`` (True) or anything else (False: the FGD encoder's path, unchanged).  Checked before anything runs: the
    net's pose width against the generator's, eval mode, a latent size ``take_distance`` can read, the stride, and the shortest track the
    generator can make (one window) against the 34 poses of a MotionAE window."""
    from .model.motion_ae import MotionAE
    if not isinstance(diversity, MotionAE):
        return False
    from . import motionfeat as MF
    _enc, D, latent = MF._encoder(diversity, f"{who}: diversity=")
    if D != seed_pose.shape[-1]:
        raise L.EgError(f"{who}: diversity=: the MotionAE takes pose_dim={D}, the generator's poses have {seed_pose.shape[-1]} columns")
    if diversity.training:
        raise L.EgError(f"{who}: diversity=: the MotionAE is not in eval mode (call .eval())")
    if latent < 4 or latent % 4:
        raise L.EgError(f"{who}: diversity=: the MotionAE's latent_dim={latent}: take_distance reads features in 16-byte groups "
                        "(a multiple of 4, >= 4)")
    if stride is None or int(stride) < 1:
        raise L.EgError(f"{who}: diversity_stride={stride} (need >= 1)")
    shortest = int(gen._origin()._cfg["frames"])
    if shortest < MF.WINDOW:
        raise L.EgError(f"{who}: diversity=: a recording of one generator window has {shortest} poses < window={MF.WINDOW} "
                        "(the MotionAE takes whole windows: no padding, no resampling)")
    return True


def _emotion_arg(who, emotion, stride, gen, vae, audio, text, seed_pose, labels, hop_samples, windows, fps, sample_rate, lengths, draws,
                 audio_rate, takes):
    """The ``emotion=`` argument of `synthesize` / `synthesize_takes`, checked before anything runs: the classifier against the generator's
    poses, and the call's own ``labels`` reduced to one class index per take -- int64 numpy ``[U, R]`` (R = 1 without draws), or None without
    a VAE or labels.  Labels that change along a take's windows are refused by name: one label per take is what is scored."""
    from . import emotion as EM
    _F, _dm, D, _C = EM._geometry(emotion, f"{who}: emotion=")
    if D != seed_pose.shape[-1]:
        raise L.EgError(f"{who}: emotion=: the classifier takes pose_dim={D}, the generator's poses have {seed_pose.shape[-1]} columns")
    if emotion.training:
        raise L.EgError(f"{who}: emotion=: the classifier is not in eval mode (call .eval())")
    if stride is not None and int(stride) < 1:
        raise L.EgError(f"{who}: emotion_stride={stride} (None or >= 1)")
    if vae is None or labels is None:
        return None
    if audio.dim() != 2:
        raise L.EgError(f"audio shape {tuple(audio.shape)} != (U, total_samples)")
    U, R = int(audio.shape[0]), 1 if draws is None else int(draws)
    cfg = gen._origin()._cfg
    if takes and lengths is None:
        lengths = [int(audio.shape[1])] * U
    if lengths is not None:                                                               # the windows of recording u, as the roll-out counts them
        hop = int(round((cfg["frames"] - cfg["prior_frames"]) * sample_rate / fps)) if hop_samples is None else int(hop_samples)
        at_model_rate = int
        if audio_rate is not None and int(audio_rate) != int(sample_rate):
            from . import resample as RS
            at_model_rate = lambda v: RS.out_length(v, int(audio_rate), int(sample_rate))
        wp = [max(1, -(-at_model_rate(v) // hop)) for v in int_list(lengths)]
    else:
        W = int(text.shape[1]) if windows is None and text.dim() == 3 else windows
        wp = [1 if W is None else max(1, int(W))] * U
    if len(wp) != U:
        raise L.EgError(f"{who}: lengths has {len(wp)} entries for {U} recordings")
    lab = np.asarray(labels.detach().cpu().numpy() if isinstance(labels, torch.Tensor) else labels)
    Wmax, N, K = max(wp), sum(wp), lab.shape[-1] if lab.ndim else 0
    off = np.concatenate([[0], np.cumsum(wp)[:-1]])
    shape = tuple(lab.shape)
    if lab.ndim == 2 and shape[0] == U:                                                   # one label per recording (U == N * R: the same rows)
        rows = lambda u, r: lab[u][None]
    elif lab.ndim == 3 and shape[0] == U and shape[1] >= Wmax:
        rows = lambda u, r: lab[u, :wp[u]]
    elif lab.ndim == 4 and shape[:2] == (U, R) and shape[2] >= Wmax:
        rows = lambda u, r: lab[u, r, :wp[u]]
    elif lab.ndim == 2 and shape[0] == N * R:                                             # packed: window w of take r of recording u at R*off[u] + r*W_u + w
        rows = lambda u, r: lab[R * off[u] + r * wp[u]: R * off[u] + (r + 1) * wp[u]]
    else:
        raise L.EgError(f"{who}: emotion=: labels shape {shape}: need ({U},K), ({U},W,K), ({U},{R},W,K) or packed ({N * R},K) one-hot rows")
    idx = np.zeros((U, R), np.int64)
    for u in range(U):
        for r in range(R):
            w = rows(u, r)
            if (w != w[:1]).any():
                raise L.EgError(f"{who}: emotion=: the labels of recording {u}, take {r} change along its windows; one label per take is what "
                                "is scored -- score the pieces with emotion.emotion_of_tracks")
            idx[u, r] = int(np.argmax(w[0]))
    return idx


def _track_outputs(who, seed_pose, *args):
    """The output stage of `synthesize` / `synthesize_takes` (skeleton.TrackOutputs, or None): their arguments, checked before anything else."""
    from . import skeleton as SK
    outs = SK.TrackOutputs(who, *args, pose_dim=seed_pose.shape[-1], hint=" (the BEAT generators' 282 columns hold rotations, not bone direction "
                           "vectors): their body is a skeleton.JointTree of 47 joints")
    return None if outs.body is None else outs


def _synthesize(who, models, audio, text, seed_pose, labels, hop_samples, n_samples, windows, z, alpha, fps, sample_rate, want_windows, want_aux,
                mel, lengths, draws, beat, diversity, audio_rate, outputs, smooth, takes, kinematics=None, srgr=None, l1div=False, emotion=None,
                emotion_stride=None, diversity_stride=34, bvh_text=None, preview=None):
    """The body of `synthesize` and `synthesize_takes` (`who` names the caller in errors): argument checks, resampling, the roll-out of the
    call's kind, then the per-track extras.  `outputs`: the caller's checked output stage (`_track_outputs`)."""
    gen, vae = models
    if smooth is not None:
        from . import smooth as SM
        smooth = SM.Smoother.of(smooth, f"{who}: smooth", fps)
        if smooth.deriv != 0:
            raise L.EgError(f"{who}: smooth=: deriv={smooth.deriv}: a velocity track is not a pose track; call smooth.smooth_tracks on "
                            "out[\"track\"] for derivatives")
    _eval_only(gen)
    if emotion is not None:                                                               # the classifier and one label per take, before anything runs
        emotion_labels = _emotion_arg(who, emotion, emotion_stride, gen, vae, audio, text, seed_pose, labels, hop_samples, windows, fps,
                                      sample_rate, lengths, draws, audio_rate, takes)
    if beat and seed_pose.shape[-1] < 174:
        raise L.EgError(f"{who}: beat=True: pose_dim={seed_pose.shape[-1]}: the beat joints are columns 18:42 and 150:174 (needs >= 174)")
    if draws is not None:
        if lengths is not None and not takes:
            raise L.EgError("synthesize: draws= with lengths= is not supported (draws in the ragged roll-out are synthesize_takes); call "
                            "synthesize_takes(..., lengths=, draws=R), or the rectangular synthesize(..., draws=R) once per group of "
                            "recordings of equal length")
        if vae is None:
            raise L.EgError(f"{who}: draws= needs a VAE (without sampled emotion maps every draw is the same track)")
        if int(draws) < 1:
            raise L.EgError(f"{who}: draws={int(draws)} (need >= 1)")
    if diversity is not None and (draws is None or int(draws) < 2):
        raise L.EgError(f"{who}: diversity= needs draws >= 2 (got draws={draws}): the take diversity is a distance between the takes of "
                        "one recording")
    motion_ae = _motion_ae_arg(who, diversity, diversity_stride, gen, seed_pose)          # a MotionAE: checked before anything runs
    eng = gen.engine()
    c = eng.cfg
    if audio.dim() != 2:
        raise L.EgError(f"audio shape {tuple(audio.shape)} != (U, total_samples)")
    U = audio.shape[0]
    if takes and lengths is None:
        lengths = [int(audio.shape[1])] * U
    resampled = audio_rate is not None and int(audio_rate) != int(sample_rate)
    if resampled:
        from . import resample as RS
        if lengths is not None:
            lengths = int_list(lengths)
    if srgr is not None or preview is not None:                                           # T' of the track this call will make: the targets' and the pictures'
        from .skeleton import out_frames
        hop = int(round((c.frames - c.prior_frames) * sample_rate / fps)) if hop_samples is None else int(hop_samples)      # _front_end's
        at_model_rate = (lambda v: RS.out_length(v, int(audio_rate), int(sample_rate))) if resampled else int
        most = max(-(-at_model_rate(v) // hop) for v in int_list(lengths)) if lengths is not None else (
            int(text.shape[1]) if windows is None and text.dim() == 3 else windows)
        if most is not None and most >= 1:                                               # otherwise the call is refused below ("windows=None"): nothing runs
            t_out = out_frames(most * (c.frames - c.prior_frames) + c.prior_frames, outputs.fps)
            if srgr is not None:
                srgr.fit(who, T=t_out)
            if preview is not None:
                preview.fit(int(U) * (1 if draws is None else max(1, int(draws))), t_out, f"{who}: preview=")
    if resampled:
        with torch.no_grad():
            audio = RS.resample_audio(audio, int(audio_rate), int(sample_rate), lengths=lengths)
        if lengths is not None:
            lengths = [RS.out_length(v, int(audio_rate), int(sample_rate)) for v in lengths]
    if takes:
        out, spec, wp = _synthesize_takes(eng, vae, audio, lengths, text, seed_pose, labels, z, alpha, want_windows, want_aux, int(draws),
                                          *_front_end(c, audio, hop_samples, n_samples, fps, sample_rate, mel))
        out["windows_per"] = wp
    elif lengths is not None:
        out, spec, wp = _synthesize_ragged(eng, vae, audio, lengths, text, seed_pose, labels, z, alpha, want_windows, want_aux,
                                           *_front_end(c, audio, hop_samples, n_samples, fps, sample_rate, mel))
        out["windows_per"] = wp
    else:
        W = int(text.shape[1]) if windows is None and text.dim() == 3 else windows
        if W is None or W < 1:
            raise L.EgError(f"windows={W} (need >= 1): text must be [U, W, {c.text_len}] or `windows` given")
        out, spec = _synthesize_rect(eng, vae, audio, W, text, seed_pose, labels, z, alpha, want_windows, want_aux, draws,
                                     *_front_end(c, audio, hop_samples, n_samples, fps, sample_rate, mel))
        wp = [W] * U
    out["spec"] = spec
    if resampled:
        out["audio"] = audio
        if lengths is not None:
            out["lengths"] = list(lengths)
    frames = [int(w) * (c.frames - c.prior_frames) + c.prior_frames for w in wp]         # recording u's own valid poses
    if beat:
        from .beat import beat_alignment_tracks
        with torch.no_grad():
            out["beat"] = beat_alignment_tracks(audio, out["track"], lengths=lengths, frames=frames, fps=fps)
    if diversity is not None:
        with torch.no_grad():
            if motion_ae:                                                                 # per 34-frame window of the TED feature space
                td = take_diversity(diversity, out["track"], frames=frames if takes else None, span=1, stride=int(diversity_stride))
            else:
                td = take_diversity(diversity, out["track"], frames=frames if takes else None, span=c.frames)
        out["take_distance"], out["take_diversity"] = td["distance"], td["diversity"]
    if emotion is not None:                                                               # of the raw track too: it measures the model
        from . import emotion as EM
        out["emotion"] = EM.emotion_of_tracks(emotion, out["track"], frames, emotion_labels, emotion_stride)
    poses = out["track"]
    if smooth is not None:                                                                # beat and diversity above score the raw track
        with torch.no_grad():
            poses = out["track_smooth"] = SM.smooth_tracks(out["track"], smooth, frames=frames)
    if outputs is not None:                                                               # joints, rotations, Euler channels: skeleton.TrackOutputs
        with torch.no_grad():
            out.update(outputs.tracks(poses, frames))
    if bvh_text is not None:                                                              # the MOTION lines of every take, made on the device
        bvh_file, frame_time = bvh_text
        out["bvh"] = bvh_file.format_tracks(out["euler"], frames=out["joint_frames"], joints=outputs.body.names, frame_time=frame_time)
    if preview is not None:                                                               # the pictures of out["joints"], one launch
        from .preview import render_joints
        with torch.no_grad():
            out["preview"] = render_joints(out["joints"], preview, out["joint_frames"])
    if kinematics is not None:                                                            # of out["joints"]: the smoothed ones with smooth=
        from . import kinematics as KN
        with torch.no_grad():
            out["kinematics"] = KN.kinematics_of_joints(out["joints"], kinematics.fps, frames=out["joint_frames"], edges=kinematics)
    if srgr is not None or l1div:                                                         # of out["joints"] too
        from . import jointscore as JS
        with torch.no_grad():
            if srgr is not None:
                there = lambda v: None if v is None else torch.as_tensor(v).to(out["joints"].device)
                out["srgr"] = JS.srgr_of_joints(out["joints"], there(srgr.joints), there(srgr.semantic), out["joint_frames"], srgr.threshold)
            if l1div:
                out["l1div"] = JS.l1div_of_tracks(out["joints"].flatten(-2), out["joint_frames"])
    return out


def _front_end(c, audio, hop_samples, n_samples, fps, sample_rate, mel):
    """(hop, n, mel): the windows' hop and length in samples (defaults from the generator's geometry) and the mel front-end."""
    from .engine import MelFrontEnd
    hop = int(round((c.frames - c.prior_frames) * sample_rate / fps)) if hop_samples is None else int(hop_samples)
    n = (c.spec_len - 1) * 512 if n_samples is None else int(n_samples)
    return hop, n, MelFrontEnd(audio.device) if mel is None else mel


def _synthesize_rect(eng, vae, audio, W, text, seed_pose, labels, z, alpha, want_windows, want_aux, draws, hop, n, mel):
    c = eng.cfg
    U = audio.shape[0]
    with torch.no_grad():
        spec = mel.windows(audio, W, hop, n, out_frames=c.spec_len)
        if draws is not None:
            R = int(draws)
            if labels is None:
                raise L.EgError("labels: needed with draws= ([U, 8], [U, W, 8] or [U, R, W, 8] one-hot)")
            lab = labels.to(audio.device)
            if tuple(lab.shape) == (U, 8):
                lab = lab[:, None, None, :].expand(U, R, W, 8)
            elif tuple(lab.shape) == (U, W, 8):
                lab = lab[:, None, :, :].expand(U, R, W, 8)
            elif tuple(lab.shape) != (U, R, W, 8):
                raise L.EgError(f"labels shape {tuple(labels.shape)}: need ({U},8), ({U},{W},8) or ({U},{R},{W},8)")
            if z is None:
                z = torch.randn(U, R, W, 32)
            elif tuple(z.shape) != (U, R, W, 32):
                raise L.EgError(f"z shape {tuple(z.shape)} != ({U},{R},{W},32)")
            sampled = vae.sample(lab.reshape(U * R * W, 8).contiguous(), z=z.reshape(U * R * W, 32)).view(U, R, W, c.frames, c.d_model)
            return eng.forward_rollout_draws(spec, text, seed_pose, sampled, alpha=alpha, want_windows=want_windows, want_aux=want_aux), spec
        sampled = None
        if vae is not None:
            if labels is None:
                raise L.EgError("labels: needed when a VAE is given ([U, 8] or [U, W, 8] one-hot)")
            lab = labels.to(audio.device)
            lab = (lab[:, None, :].expand(U, W, 8) if lab.dim() == 2 else lab).reshape(U * W, 8).contiguous()
            sampled = vae.sample(lab, z=None if z is None else z.reshape(U * W, 32)).view(U, W, c.frames, c.d_model)
        return eng.forward_rollout(spec, text, seed_pose, sampled, alpha=alpha, want_windows=want_windows, want_aux=want_aux), spec


def _synthesize_ragged(eng, vae, audio, lengths, text, seed_pose, labels, z, alpha, want_windows, want_aux, hop, n, mel):
    c = eng.cfg
    U = audio.shape[0]
    with torch.no_grad():
        spec, wp = mel.windows_ragged(audio, lengths, hop, n, out_frames=c.spec_len)
        N = sum(wp)
        packed = lambda x, packed_dim, name: eng.pack_ragged(x, wp, name) if x.dim() == packed_dim + 1 else x
        sampled = None
        if vae is not None:
            if labels is None:
                raise L.EgError("labels: needed when a VAE is given ([U, 8], [U, Wmax, 8] or packed [N, 8] one-hot)")
            lab = labels.to(audio.device).float()
            if lab.dim() == 2 and lab.shape[0] == U and U != N:         # one label per recording: repeated over its windows
                lab = lab[:, None, :].expand(U, max(wp), 8).contiguous()
            lab = packed(lab, 2, "labels")
            if tuple(lab.shape) != (N, 8):
                raise L.EgError(f"labels shape {tuple(labels.shape)}: need ({U},8), ({U},{max(wp)},8) or packed ({N},8)")
            if z is not None:
                z = packed(z.to(audio.device).float(), 2, "z")
                if tuple(z.shape) != (N, 32):
                    raise L.EgError(f"z shape {tuple(z.shape)}: need ({U},{max(wp)},32) or packed ({N},32)")
            sampled = vae.sample(lab, z=z)
        out = eng.forward_rollout_ragged(spec, packed(text, 2, "text"), seed_pose, wp, sampled, alpha=alpha, want_windows=want_windows,
                                         want_aux=want_aux)
    return out, spec, list(wp)


def _synthesize_takes(eng, vae, audio, lengths, text, seed_pose, labels, z, alpha, want_windows, want_aux, R, hop, n, mel):
    c = eng.cfg
    U = audio.shape[0]
    with torch.no_grad():
        spec, wp = mel.windows_ragged(audio, lengths, hop, n, out_frames=c.spec_len)
        wp = tuple(wp)
        N, Wmax = sum(wp), max(wp)
        per_take = tuple(w for w in wp for _ in range(R))           # [U, R, Wmax, ...] viewed as U*R padded recordings: the packed take order
        pack_takes = lambda x, name: eng.pack_ragged(x.reshape((U * R, Wmax) + tuple(x.shape[3:])).contiguous(), per_take, name)
        if labels is None:
            raise L.EgError("labels: needed with draws= ([U, 8], [U, Wmax, 8], [U, R, Wmax, 8] or packed [N*R, 8] one-hot)")
        lab = labels.to(audio.device).float()
        if tuple(lab.shape) != (N * R, 8):
            if tuple(lab.shape) == (U, 8):
                lab = lab[:, None, None, :].expand(U, R, Wmax, 8)
            elif tuple(lab.shape) == (U, Wmax, 8):
                lab = lab[:, None, :, :].expand(U, R, Wmax, 8)
            elif tuple(lab.shape) != (U, R, Wmax, 8):
                raise L.EgError(f"labels shape {tuple(labels.shape)}: need ({U},8), ({U},{Wmax},8), ({U},{R},{Wmax},8) or packed ({N * R},8)")
            lab = pack_takes(lab, "labels")
        if z is None:
            z = torch.randn(N * R, 32)
        elif tuple(z.shape) == (U, R, Wmax, 32):
            z = pack_takes(z.to(audio.device).float(), "z")
        elif tuple(z.shape) != (N * R, 32):
            raise L.EgError(f"z shape {tuple(z.shape)}: need ({U},{R},{Wmax},32) or packed ({N * R},32)")
        sampled = vae.sample(lab.contiguous(), z=z)
        out = eng.forward_rollout_takes(spec, eng.pack_ragged(text, wp, "text") if text.dim() == 3 else text, seed_pose, wp, sampled,
                                        alpha=alpha, want_windows=want_windows, want_aux=want_aux)
    return out, spec, list(wp)


def open_stream(models, rows: int, seed_pose: torch.Tensor, *, mel=None, **kw):
    """`synthesize` fed hop by hop: a `streaming.GestureStream` for `rows` speakers.  ``models = (generator, vae | None)``, eval mode, on the GPU;
    ``mel``: a MelFrontEnd to share (default: one of the session's own on seed_pose's device), as for `synthesize`.  A row's emitted rows followed
    by its tail are `synthesize`'s track for the same audio, text, labels / z, seed pose and alpha.  Sessions on ready spectrograms (push_spec):
    `streaming.GestureStream((generator, vae, None), ...)`."""
    from .streaming import AUTO_MEL, GestureStream
    gen, vae = models
    return GestureStream((gen, vae, AUTO_MEL if mel is None else mel), rows, seed_pose, **kw)
