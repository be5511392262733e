"""Device-side engines: a packed weight arena + workspace + one C-ABI call per batch.

PyTorch is used here only for device memory (arena / workspace / outputs come from its caching
allocator) and for the current HIP stream; every FLOP of the path runs in libemogest_hip.so.
"""
from __future__ import annotations

import ctypes as C
import functools
import threading
from typing import Dict, Mapping, Optional

import torch

from . import _lib as L
from . import packing
from ._host import BoundedCache, host_ptr, int_list
from ._host import need_cuda as _need_cuda, ptr as _ptr, stream as _stream      # these names stay importable from here (tests, tools)


def _locked(fn):
    """Serialise the host-side enqueue of one engine: a call carves the engine's workspace and enqueues ~200 kernels on the current stream;
    two threads on one device (nn.DataParallel replicas, device_ids with repeats) must not interleave theirs."""
    @functools.wraps(fn)
    def wrapper(self, *a, **k):
        with self._lock:
            return fn(self, *a, **k)
    return wrapper


def ragged_plan(windows_per) -> dict:
    """eg_rollout_ragged_plan on the host (no GPU needed): for window counts W_u the working order "longer first, ties by index" (`order`:
    rank -> recording, `inverse`: recording -> rank), `step_batch` [Wmax] (recordings active in step s), `offsets` [U] (exclusive prefix
    sum of W_u: recording u's first packed row), `slot_row` [N] (step-major slot -> packed row) and `table` [N + 2U], what the device reads."""
    import numpy as np
    wp = np.ascontiguousarray(np.asarray(windows_per, dtype=np.int32).reshape(-1))
    lib = L.load()
    U = int(wp.size)
    N = int(wp.astype(np.int64).sum()) if U else 0
    good = U >= 1 and bool((wp >= 1).all())
    Wmax = int(wp.max()) if good else 1
    ints = lib.eg_rollout_ragged_plan_ints(U, N) if good else 0
    order, inverse = np.zeros(max(U, 1), np.int32), np.zeros(max(U, 1), np.int32)
    step_batch, table = np.zeros(Wmax, np.int32), np.zeros(max(int(ints), 1), np.int32)
    p = host_ptr
    L.check(lib.eg_rollout_ragged_plan(p(wp), U, p(order), p(inverse), p(step_batch), p(table) if ints > 0 else None), "eg_rollout_ragged_plan")
    if ints <= 0:
        raise L.EgError(f"eg_rollout_ragged_plan_ints: unsupported U={U} N={N}")
    offsets = np.concatenate([[0], np.cumsum(wp[:-1], dtype=np.int64)]).astype(np.int32)
    return {"windows_per": wp, "order": order, "inverse": inverse, "step_batch": step_batch, "offsets": offsets, "slot_row": table[:N].copy(),
            "table": table}


class GeneratorEngine:
    """Host handle for eg_generator_* (Transformer.forward, Full_model/Models_spatial_memory.py:566-616)."""

    def __init__(self, *, frames=34, pose_dim=126, prior_frames=4, chunk=4, d_model=512, d_inner=2048, n_layers=3,
                 n_head=8, d_k=64, n_mels=128, spec_len=124, text_len=60, n_words=200, embed_dim=300, tcn_hidden=300,
                 tcn_layers=3, variant="spatial", precision="f32", n_position=60, keep_taps=False, concurrent=False, fold_affine=False, fuse_se=True,
                 shared_chip=False):
        lib = L.load()
        cfg = L.EgGeneratorConfig()
        L.check(lib.eg_generator_default_config(C.byref(cfg)), "eg_generator_default_config")
        cfg.frames, cfg.pose_dim, cfg.prior_frames, cfg.chunk = frames, pose_dim, prior_frames, chunk
        cfg.d_model, cfg.d_inner, cfg.n_layers, cfg.n_head, cfg.d_k = d_model, d_inner, n_layers, n_head, d_k
        cfg.n_mels, cfg.spec_len, cfg.text_len, cfg.n_words = n_mels, spec_len, text_len, n_words
        cfg.embed_dim, cfg.tcn_hidden, cfg.tcn_layers = embed_dim, tcn_hidden, tcn_layers
        cfg.variant = {"spatial": 0, "memory": 1}[variant] if isinstance(variant, str) else int(variant)
        cfg.precision = L.precision_code(precision)
        cfg.n_position = max(n_position, frames)
        cfg.reserved[0] = 1 if keep_taps else 0
        cfg.reserved[1] = 1 if concurrent else 0
        cfg.reserved[2] = 1 if fold_affine else 0
        cfg.reserved[3] = 0 if fuse_se else 1
        cfg.reserved[4] = 1 if shared_chip else 0     # several batches in flight (ClipPipeline): GEMM tiles chosen for CU time, not latency
        self.cfg = cfg
        h = C.c_void_p()
        L.check(lib.eg_generator_create(C.byref(cfg), C.byref(h)), "eg_generator_create")
        self._h = h
        self._lib = lib
        self.entries = packing.manifest(h, "eg_generator_num_weights", "eg_generator_weight_entry")
        self.arena_floats = lib.eg_generator_arena_floats(h)
        self.arena: Optional[torch.Tensor] = None
        self._ws: Dict[tuple, torch.Tensor] = {}
        self._plans = BoundedCache(64)          # ragged roll-out: plan tables per (W_u) vector and device; a long-running caller with ever-new
        #                                         vectors drops the oldest
        self._lock = threading.RLock()
        self.uploads = 0                 # arena packs + uploads so far (tests: once per device and weight version)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._lib.eg_generator_destroy(self._h)
                self._h = None
        except Exception:
            pass

    # ---- weights ----
    def load_weights(self, sd: Mapping[str, torch.Tensor], device) -> None:
        cpu = packing.build_arena(packing.strip_module_prefix(sd), self.entries, self.arena_floats)
        with self._lock:
            self.arena = cpu.to(device)
            self._ws.clear()
            self.uploads += 1

    def _workspace(self, key, nbytes: int, device) -> torch.Tensor:
        ws = self._ws.get(key)
        if ws is None or ws.numel() < nbytes or ws.device != torch.device(device):
            ws = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
            self._ws[key] = ws
        return ws

    # ---- Transformer.forward ----
    @_locked
    def forward(self, spec, text, prior, sampled=None, want_aux=True, slot=0):
        if self.arena is None:
            raise L.EgError("GeneratorEngine.forward before load_weights")
        dev = self.arena.device
        c = self.cfg
        spec = _need_cuda(spec, "input_spectrum")
        text = _need_cuda(text, "text", torch.int64)
        prior = _need_cuda(prior, "prior_seq")
        B = spec.shape[0]
        if tuple(spec.shape) != (B, c.n_mels, c.spec_len):
            raise L.EgError(f"input_spectrum shape {tuple(spec.shape)} != (B,{c.n_mels},{c.spec_len})")
        if tuple(text.shape) != (B, c.text_len):
            raise L.EgError(f"text shape {tuple(text.shape)} != (B,{c.text_len})")
        if tuple(prior.shape) != (B, c.prior_frames, c.pose_dim):
            raise L.EgError(f"prior_seq shape {tuple(prior.shape)} != (B,{c.prior_frames},{c.pose_dim})")
        if sampled is not None:
            sampled = _need_cuda(sampled, "sampled_emotion_feature")
            if tuple(sampled.shape) != (B, c.frames, c.d_model):
                raise L.EgError(f"sampled_emotion_feature shape {tuple(sampled.shape)} != (B,{c.frames},{c.d_model})")
        ws_bytes = self._lib.eg_generator_workspace_bytes(self._h, B)
        ws = self._workspace(("fwd", B) if slot == 0 else ("fwd", B, slot), ws_bytes, dev)   # one workspace per concurrent slot
        pose = torch.empty(B, c.frames, c.pose_dim, device=dev)
        emo = torch.empty(B, c.frames, c.d_model, device=dev) if want_aux else None
        sem = torch.empty(B, c.frames, c.d_model, device=dev) if want_aux else None
        pred = torch.empty(B, 8, device=dev) if want_aux else None
        txt = torch.empty(B, c.text_len, 512, device=dev) if want_aux else None
        L.check(self._lib.eg_generator_forward(self._h, _ptr(self.arena), B, _ptr(spec), _ptr(text), _ptr(prior), _ptr(sampled),
                                               _ptr(pose), _ptr(emo), _ptr(sem), _ptr(pred), _ptr(txt), _ptr(ws), ws_bytes,
                                               _stream(dev)), "eg_generator_forward")
        return pose, emo, sem, pred, txt

    @_locked
    def forward_draws(self, spec, prior, sampled, slot=0):
        """BASELINE config 5: sampled [B, R, frames, d_model] -> pose [B, R, frames, pose_dim].  slot: a private workspace (one per step in flight)."""
        dev = self.arena.device
        c = self.cfg
        spec, prior, sampled = _need_cuda(spec, "spec"), _need_cuda(prior, "prior"), _need_cuda(sampled, "sampled")
        B, R = sampled.shape[0], sampled.shape[1]
        ws_bytes = self._lib.eg_generator_draws_workspace_bytes(self._h, B, R)
        ws = self._workspace(("draws", B, R) if slot == 0 else ("draws", B, R, slot), ws_bytes, dev)
        pose = torch.empty(B, R, c.frames, c.pose_dim, device=dev)
        L.check(self._lib.eg_generator_forward_draws(self._h, _ptr(self.arena), B, R, _ptr(spec), _ptr(prior), _ptr(sampled),
                                                     _ptr(pose), _ptr(ws), ws_bytes, _stream(dev)), "eg_generator_forward_draws")
        return pose

    # ---- long-form synthesis: what the three roll-out calls share ----
    def _loaded(self, method: str):
        """The weights' device; `method` names the caller in the error."""
        if self.arena is None:
            raise L.EgError(f"GeneratorEngine.{method} before load_weights")
        return self.arena.device

    @staticmethod
    def _rollout_tensors(spec, text, seed_pose, sampled, alpha):
        return (_need_cuda(spec, "spec"), _need_cuda(text, "text", torch.int64), _need_cuda(seed_pose, "seed_pose"),
                None if sampled is None else _need_cuda(sampled, "sampled"), None if alpha is None else _need_cuda(alpha, "alpha"))

    def _rollout_workspace(self, kind: str, fn: str, sizes: dict, slot, dev):
        """(workspace, bytes) of one roll-out call: `fn` is the C query, `sizes` its named arguments, (kind, *sizes[, slot]) the slot key."""
        ws_bytes = getattr(self._lib, fn)(self._h, *sizes.values())
        if ws_bytes <= 0:
            raise L.EgError(f"{fn}: unsupported " + " ".join(f"{k}={v}" for k, v in sizes.items()))
        key = (kind, *sizes.values())
        return self._workspace(key if slot == 0 else key + (slot,), ws_bytes, dev), ws_bytes

    def _rollout_outputs(self, dev, track_lead, steps, windows_lead, clip_lead, want_windows, want_aux, track=None):
        """The output dictionary: track [*track_lead, steps*(F-P)+P, D], windows [*windows_lead, F, D], per-window outputs [*clip_lead, ...]."""
        c = self.cfg
        T = steps * (c.frames - c.prior_frames) + c.prior_frames
        out = {"track": torch.empty(*track_lead, T, c.pose_dim, device=dev) if track is None else track,
               "emotion_prediction": torch.empty(*clip_lead, 8, device=dev)}
        if want_windows:
            out["windows"] = torch.empty(*windows_lead, c.frames, c.pose_dim, device=dev)
        if want_aux:
            out["emotion_feature"] = torch.empty(*clip_lead, c.frames, c.d_model, device=dev)
            out["semantic_feature"] = torch.empty(*clip_lead, c.frames, c.d_model, device=dev)
            out["text_embedding"] = torch.empty(*clip_lead, c.text_len, 512, device=dev)
        return out

    def _rollout_call(self, fn: str, sizes, tensors, out, ws, ws_bytes, dev):
        """The C call: handle, arena, the call's own size / plan arguments, then what every roll-out entry takes in the same order."""
        L.check(getattr(self._lib, fn)(
            self._h, _ptr(self.arena), *sizes, *(_ptr(t) for t in tensors), _ptr(out["track"]), _ptr(out.get("windows")),
            _ptr(out["emotion_prediction"]), _ptr(out.get("emotion_feature")), _ptr(out.get("semantic_feature")), _ptr(out.get("text_embedding")),
            _ptr(ws), ws_bytes, _stream(dev)), fn)
        return out

    def _rollout_args(self, spec, text, seed_pose, sampled, alpha):
        """Shape contract of forward_rollout (checked before anything touches the device); returns (U, W)."""
        c = self.cfg
        if spec.dim() != 4 or tuple(spec.shape[2:]) != (c.n_mels, c.spec_len):
            raise L.EgError(f"spec shape {tuple(spec.shape)} != (U,W,{c.n_mels},{c.spec_len})")
        U, W = int(spec.shape[0]), int(spec.shape[1])
        if U < 1:
            raise L.EgError(f"spec: utterances U={U} (need >= 1)")
        if W < 1:
            raise L.EgError(f"spec: windows W={W} (need >= 1)")
        if tuple(text.shape) != (U, W, c.text_len):
            raise L.EgError(f"text shape {tuple(text.shape)} != ({U},{W},{c.text_len})")
        if tuple(seed_pose.shape) != (U, c.prior_frames, c.pose_dim):
            raise L.EgError(f"seed_pose shape {tuple(seed_pose.shape)} != ({U},{c.prior_frames},{c.pose_dim})")
        if sampled is not None and tuple(sampled.shape) != (U, W, c.frames, c.d_model):
            raise L.EgError(f"sampled shape {tuple(sampled.shape)} != ({U},{W},{c.frames},{c.d_model})")
        if alpha is not None and tuple(alpha.shape) != (c.prior_frames,):
            raise L.EgError(f"alpha shape {tuple(alpha.shape)} != ({c.prior_frames},)")
        return U, W

    @_locked
    def forward_rollout(self, spec, text, seed_pose, sampled=None, alpha=None, want_windows=False, want_aux=False, slot=0):
        """eg_generator_forward_rollout: W consecutive windows of U utterances, each seeded with the raw last prior_frames poses of the one
        before it, stitched into one track with a linear cross-fade over the overlap.
        spec [U,W,n_mels,spec_len], text [U,W,text_len], seed_pose [U,P,D], sampled [U,W,F,d_model] or None, alpha [P] or None
        (alpha[j] = (j+1)/(P+1)).  Returns a dict: track [U, W*(F-P)+P, D], emotion_prediction [U,W,8], windows [U,W,F,D] with
        want_windows, emotion_feature / semantic_feature [U,W,F,d_model] and text_embedding [U,W,text_len,512] with want_aux."""
        U, W = self._rollout_args(spec, text, seed_pose, sampled, alpha)
        dev = self._loaded("forward_rollout")
        tensors = self._rollout_tensors(spec, text, seed_pose, sampled, alpha)
        ws, ws_bytes = self._rollout_workspace("rollout", "eg_generator_rollout_workspace_bytes", {"U": U, "W": W}, slot, dev)
        out = self._rollout_outputs(dev, (U,), W, (U, W), (U, W), want_windows, want_aux)
        return self._rollout_call("eg_generator_forward_rollout", (U, W), tensors, out, ws, ws_bytes, dev)

    # ---- diverse roll-out: several sampled tracks per recording ----
    def _rollout_draws_args(self, spec, text, seed_pose, sampled, alpha):
        """Shape contract of forward_rollout_draws (checked before anything touches the device); returns (U, W, R)."""
        c = self.cfg
        if sampled is None:
            raise L.EgError(f"sampled: required, shape (U,R,W,F,d_model) = (U,R,W,{c.frames},{c.d_model}) (without it every draw is the same track)")
        if sampled.dim() != 5:
            raise L.EgError(f"sampled shape {tuple(sampled.shape)} != (U,R,W,F,d_model) = (U,R,W,{c.frames},{c.d_model})")
        R = int(sampled.shape[1])
        if R < 1:
            raise L.EgError(f"sampled shape {tuple(sampled.shape)}: draws R={R} (need >= 1) in (U,R,W,F,d_model)")
        U, W = self._rollout_args(spec, text, seed_pose, None, alpha)
        if tuple(sampled.shape) != (U, R, W, c.frames, c.d_model):
            raise L.EgError(f"sampled shape {tuple(sampled.shape)} != (U,R,W,F,d_model) = ({U},{R},{W},{c.frames},{c.d_model})")
        return U, W, R

    @_locked
    def forward_rollout_draws(self, spec, text, seed_pose, sampled, alpha=None, want_windows=False, want_aux=False, slot=0):
        """eg_generator_forward_rollout_draws: R sampled tracks for each of U recordings, the audio tower run once per window.  By definition
        forward_rollout on U*R recordings, recording u*R + r having spec[u], text[u], seed_pose[u] and sampled[u, r].
        spec [U,W,n_mels,spec_len], text [U,W,text_len], seed_pose [U,P,D], sampled [U,R,W,F,d_model] (required), alpha [P] or None.
        Returns a dict: track [U, R, W*(F-P)+P, D], emotion_prediction [U,W,8] (independent of the draw), windows [U,R,W,F,D] with
        want_windows, emotion_feature / semantic_feature [U,W,F,d_model] and text_embedding [U,W,text_len,512] with want_aux."""
        U, W, R = self._rollout_draws_args(spec, text, seed_pose, sampled, alpha)
        dev = self._loaded("forward_rollout_draws")
        tensors = self._rollout_tensors(spec, text, seed_pose, sampled, alpha)
        ws, ws_bytes = self._rollout_workspace("rollout_draws", "eg_generator_rollout_draws_workspace_bytes", {"U": U, "W": W, "R": R}, slot, dev)
        out = self._rollout_outputs(dev, (U, R), W, (U, R, W), (U, W), want_windows, want_aux)
        return self._rollout_call("eg_generator_forward_rollout_draws", (U, W, R), tensors, out, ws, ws_bytes, dev)

    # ---- ragged roll-out: recordings with their own window counts ----
    def _rollout_ragged_args(self, spec, text, seed_pose, windows_per, sampled, alpha):
        """Shape contract of forward_rollout_ragged (checked before anything touches the device); returns (U, N, windows_per as a tuple)."""
        c = self.cfg
        try:
            wp = tuple(int_list(windows_per))
        except TypeError:
            raise L.EgError(f"windows_per: need a sequence of U window counts (got {type(windows_per).__name__})")
        U = len(wp)
        if U < 1:
            raise L.EgError(f"windows_per: utterances U={U} (need >= 1)")
        for u, v in enumerate(wp):
            if v < 1:
                raise L.EgError(f"windows_per[{u}]={v} (need >= 1)")
        N = sum(wp)
        if N > 1 << 20:
            raise L.EgError(f"windows_per: total windows N={N} > 2^20")
        if tuple(spec.shape) != (N, c.n_mels, c.spec_len):
            raise L.EgError(f"spec shape {tuple(spec.shape)} != (N={N},{c.n_mels},{c.spec_len}) packed, N = sum(windows_per)")
        if tuple(text.shape) != (N, c.text_len):
            raise L.EgError(f"text shape {tuple(text.shape)} != ({N},{c.text_len})")
        if tuple(seed_pose.shape) != (U, c.prior_frames, c.pose_dim):
            raise L.EgError(f"seed_pose shape {tuple(seed_pose.shape)} != ({U},{c.prior_frames},{c.pose_dim})")
        if sampled is not None and tuple(sampled.shape) != (N, c.frames, c.d_model):
            raise L.EgError(f"sampled shape {tuple(sampled.shape)} != ({N},{c.frames},{c.d_model})")
        if alpha is not None and tuple(alpha.shape) != (c.prior_frames,):
            raise L.EgError(f"alpha shape {tuple(alpha.shape)} != ({c.prior_frames},)")
        return U, N, wp

    def _ragged_plan(self, wp, device):
        """The plan of one (W_u) vector: host tables from eg_rollout_ragged_plan, the device copy of its table uploaded once and kept."""
        def build():
            ent = ragged_plan(wp)
            ent["windows_per_c"] = (C.c_int32 * len(wp))(*wp)
            ent["table_dev"] = torch.from_numpy(ent["table"]).to(device)
            return ent
        return self._plans.get((wp, str(device)), build)

    @_locked
    def pack_ragged(self, x, windows_per, name="argument"):
        """Padded [U, Wmax, ...] -> packed [N, ...] on the device by eg_rows_by_table (row off[u] + w = x[u, w] for w < W_u; entries past W_u
        are never read).  float32 or int64."""
        wp = tuple(int_list(windows_per))
        U, Wmax = len(wp), max(wp) if len(wp) else 0
        if x.dim() < 2 or int(x.shape[0]) != U or int(x.shape[1]) != Wmax:
            raise L.EgError(f"{name} shape {tuple(x.shape)}: a padded argument is (U={U}, Wmax={Wmax}, ...)")
        if self.arena is None:
            raise L.EgError("GeneratorEngine.pack_ragged before load_weights")
        x = _need_cuda(x, name, torch.int64 if x.dtype == torch.int64 else torch.float32)
        plan = self._ragged_plan(wp, x.device)
        if "pad_table_dev" not in plan:
            plan["pad_table_dev"] = torch.tensor([u * Wmax + w for u in range(U) for w in range(wp[u])], dtype=torch.int32).to(x.device)
        N = sum(wp)
        out = torch.empty((N,) + tuple(x.shape[2:]), dtype=x.dtype, device=x.device)
        words = (x[0, 0].numel() * x.element_size()) // 4
        L.check(self._lib.eg_rows_by_table(_ptr(x), _ptr(out), _ptr(plan["pad_table_dev"]), N, words, 0, _stream(x.device)), "eg_rows_by_table")
        return out

    @_locked
    def forward_rollout_ragged(self, spec, text, seed_pose, windows_per, sampled=None, alpha=None, want_windows=False, want_aux=False, slot=0,
                               track=None):
        """eg_generator_forward_rollout_ragged: U recordings with their own window counts windows_per[u] = W_u >= 1 in one call; step s runs
        the recordings with W_u > s only.  Window-indexed arguments are PACKED recording-major (N = sum W_u rows, recording u at rows
        [off[u], off[u] + W_u)): spec [N,n_mels,spec_len], text [N,text_len], sampled [N,F,d_model] or None; seed_pose [U,P,D]; alpha [P] or
        None.  Returns a dict: track [U, Wmax*(F-P)+P, D] (rows past track_frames[u] are zero), track_frames [U] = W_u*(F-P)+P and
        window_offsets [U] = off (int64, on the host), packed emotion_prediction [N,8], windows [N,F,D] with want_windows,
        emotion_feature / semantic_feature [N,F,d_model] and text_embedding [N,text_len,512] with want_aux.  `track`: a caller-owned
        contiguous float32 GPU buffer of the track's shape to write into (default: a new one); every element of it is written."""
        U, N, wp = self._rollout_ragged_args(spec, text, seed_pose, windows_per, sampled, alpha)
        T = max(wp) * (self.cfg.frames - self.cfg.prior_frames) + self.cfg.prior_frames
        if track is not None and (tuple(track.shape) != (U, T, self.cfg.pose_dim) or track.dtype != torch.float32 or not track.is_contiguous()
                                  or not track.is_cuda):
            raise L.EgError(f"track: need a contiguous float32 GPU tensor [{U},{T},{self.cfg.pose_dim}]")
        dev = self._loaded("forward_rollout_ragged")
        c = self.cfg
        tensors = self._rollout_tensors(spec, text, seed_pose, sampled, alpha)
        plan = self._ragged_plan(wp, dev)
        ws, ws_bytes = self._rollout_workspace("ragged", "eg_generator_rollout_ragged_workspace_bytes", {"U": U, "N": N}, slot, dev)
        out = self._rollout_outputs(dev, (U,), max(wp), (N,), (N,), want_windows, want_aux, track)
        out["track_frames"] = torch.tensor([v * (c.frames - c.prior_frames) + c.prior_frames for v in wp], dtype=torch.int64)
        out["window_offsets"] = torch.from_numpy(plan["offsets"].astype("int64"))
        return self._rollout_call("eg_generator_forward_rollout_ragged", (U, plan["windows_per_c"], _ptr(plan["table_dev"])), tensors, out, ws,
                                  ws_bytes, dev)

    # ---- takes: several sampled tracks per recording, recordings with their own window counts ----
    def _rollout_takes_args(self, spec, text, seed_pose, windows_per, sampled, alpha):
        """Shape contract of forward_rollout_takes (checked before anything touches the device); returns (U, N, R, windows_per as a tuple)."""
        c = self.cfg
        U, N, wp = self._rollout_ragged_args(spec, text, seed_pose, windows_per, None, alpha)
        if sampled is None:
            raise L.EgError(f"sampled: required, shape (N*R,F,d_model) = ({N}*R,{c.frames},{c.d_model}) (without it every draw is the same track)")
        if sampled.dim() != 3 or tuple(sampled.shape[1:]) != (c.frames, c.d_model) or int(sampled.shape[0]) < N or int(sampled.shape[0]) % N:
            raise L.EgError(f"sampled shape {tuple(sampled.shape)} != (N*R,F,d_model) = ({N}*R,{c.frames},{c.d_model}) packed, R >= 1 draws")
        R = int(sampled.shape[0]) // N
        if N * R > 1 << 20:
            raise L.EgError(f"sampled: windows*draws N*R={N}*{R} > 2^20")
        return U, N, R, wp

    def _takes_plan(self, wp, device):
        """The takes plan of one (W_u) vector (eg_rollout_takes_plan: the ragged table, then slot_rank), uploaded once and kept like _ragged_plan's."""
        def build():
            import numpy as np
            U, N = len(wp), sum(wp)
            w = np.asarray(wp, np.int32)
            table = np.zeros(int(self._lib.eg_rollout_takes_plan_ints(U, N)), np.int32)
            L.check(self._lib.eg_rollout_takes_plan(host_ptr(w), U, None, None, None, host_ptr(table)), "eg_rollout_takes_plan")
            off = np.concatenate([[0], np.cumsum(w[:-1], dtype=np.int64)]).astype(np.int64)
            return {"table": table, "offsets": off, "windows_per_c": (C.c_int32 * U)(*wp), "table_dev": torch.from_numpy(table).to(device)}
        return self._plans.get(("takes", wp, str(device)), build)

    @_locked
    def forward_rollout_takes(self, spec, text, seed_pose, windows_per, sampled, alpha=None, want_windows=False, want_aux=False, slot=0,
                              track=None):
        """eg_generator_forward_rollout_takes: R sampled tracks for each of U recordings with their own window counts windows_per[u] = W_u,
        the audio tower run once per window.  By definition forward_rollout_ragged on U*R recordings, recording u*R + r having the windows,
        text, seed pose and W_u of u and its own sampled maps.  spec [N,n_mels,spec_len], text [N,text_len] packed recording-major (N = sum
        W_u, off its exclusive prefix sum), seed_pose [U,P,D], sampled [N*R,F,d_model] (required; R is read from it) in the packed order of
        the replicated call -- window w of draw r of recording u is row R*off[u] + r*W_u + w --, alpha [P] or None.  Returns a dict: track
        [U, R, Wmax*(F-P)+P, D] (rows past track_frames[u] are zero), track_frames [U], window_offsets [U] = off and take_window_offsets
        [U, R] = R*off[u] + r*W_u (int64, on the host), packed emotion_prediction [N,8] (independent of the draw), windows [N*R,F,D] in the
        order of `sampled` with want_windows, emotion_feature / semantic_feature [N,F,d_model] and text_embedding [N,text_len,512] with
        want_aux.  `track`: a caller-owned contiguous float32 GPU buffer of the track's shape (default: a new one); every element is written."""
        U, N, R, wp = self._rollout_takes_args(spec, text, seed_pose, windows_per, sampled, alpha)
        c = self.cfg
        H = c.frames - c.prior_frames
        T = max(wp) * H + c.prior_frames
        if track is not None and (tuple(track.shape) != (U, R, T, c.pose_dim) or track.dtype != torch.float32 or not track.is_contiguous()
                                  or not track.is_cuda):
            raise L.EgError(f"track: need a contiguous float32 GPU tensor [{U},{R},{T},{c.pose_dim}]")
        dev = self._loaded("forward_rollout_takes")
        tensors = self._rollout_tensors(spec, text, seed_pose, sampled, alpha)
        plan = self._takes_plan(wp, dev)
        ws, ws_bytes = self._rollout_workspace("takes", "eg_generator_rollout_takes_workspace_bytes", {"U": U, "N": N, "R": R}, slot, dev)
        out = self._rollout_outputs(dev, (U, R), max(wp), (N * R,), (N,), want_windows, want_aux, track)
        off = torch.from_numpy(plan["offsets"])
        w = torch.tensor(wp, dtype=torch.int64)
        out["track_frames"] = w * H + c.prior_frames
        out["window_offsets"] = off.clone()
        out["take_window_offsets"] = R * off[:, None] + torch.arange(R, dtype=torch.int64)[None, :] * w[:, None]
        return self._rollout_call("eg_generator_forward_rollout_takes", (U, R, plan["windows_per_c"], _ptr(plan["table_dev"])), tensors, out, ws,
                                  ws_bytes, dev)

    # ---- streaming synthesis (a session's state buffer is owned by the caller: emotiongestures_amd.streaming.GestureStream) ----
    def _stream_geometry(self, rows, hop_samples, n_samples):
        if int(rows) < 1 or int(hop_samples) < 1 or int(n_samples) < 1:
            raise L.EgError(f"stream: rows={rows} hop_samples={hop_samples} n_samples={n_samples} (need >= 1)")
        return int(rows), int(hop_samples), int(n_samples)

    def _stream_state(self, state, geom):
        nbytes = self.stream_state_bytes(*geom)
        if not isinstance(state, torch.Tensor) or not state.is_cuda:
            raise L.EgError("stream state: the HIP path needs a GPU buffer (torch.uint8, stream_state_bytes long); there is no CPU fallback")
        if state.dtype != torch.uint8 or state.numel() < nbytes or not state.is_contiguous():
            raise L.EgError(f"stream state: need a contiguous uint8 buffer of {nbytes} bytes (got {state.dtype}, {state.numel()})")
        return state

    def stream_state_bytes(self, rows, hop_samples, n_samples) -> int:
        geom = self._stream_geometry(rows, hop_samples, n_samples)
        nbytes = self._lib.eg_stream_state_bytes(self._h, *geom)
        if nbytes <= 0:
            raise L.EgError(f"eg_stream_state_bytes: unsupported rows={geom[0]} hop_samples={geom[1]} n_samples={geom[2]}")
        return int(nbytes)

    def _stream_step_args(self, U, spec, text, sampled, alpha):
        """Shape contract of stream_step (checked before anything touches the device)."""
        c = self.cfg
        if tuple(spec.shape) != (U, c.n_mels, c.spec_len):
            raise L.EgError(f"spec shape {tuple(spec.shape)} != ({U},{c.n_mels},{c.spec_len})")
        if text is not None and tuple(text.shape) != (U, c.text_len):
            raise L.EgError(f"text shape {tuple(text.shape)} != ({U},{c.text_len})")
        if sampled is not None and tuple(sampled.shape) != (U, c.frames, c.d_model):
            raise L.EgError(f"sampled shape {tuple(sampled.shape)} != ({U},{c.frames},{c.d_model})")
        if alpha is not None and tuple(alpha.shape) != (c.prior_frames,):
            raise L.EgError(f"alpha shape {tuple(alpha.shape)} != ({c.prior_frames},)")

    @_locked
    def stream_reset(self, state, rows, hop_samples, n_samples, seed_pose, row_mask=None):
        """eg_stream_reset: seed_pose [U,P,D]; row_mask int32 [U] on the device (non-zero = reset that row) or None for every row."""
        geom = self._stream_geometry(rows, hop_samples, n_samples)
        c = self.cfg
        if tuple(seed_pose.shape) != (geom[0], c.prior_frames, c.pose_dim):
            raise L.EgError(f"seed_pose shape {tuple(seed_pose.shape)} != ({geom[0]},{c.prior_frames},{c.pose_dim})")
        if row_mask is not None and tuple(row_mask.shape) != (geom[0],):
            raise L.EgError(f"row_mask shape {tuple(row_mask.shape)} != ({geom[0]},)")
        state = self._stream_state(state, geom)
        seed_pose = _need_cuda(seed_pose, "seed_pose")
        row_mask = None if row_mask is None else _need_cuda(row_mask, "row_mask", torch.int32)
        L.check(self._lib.eg_stream_reset(self._h, _ptr(state), *geom, _ptr(row_mask), _ptr(seed_pose), _stream(state.device)), "eg_stream_reset")

    @_locked
    def stream_push(self, state, rows, hop_samples, n_samples, chunk, ends=None, clips=None):
        """eg_stream_push: chunk [U,hop], ends int32 [U] on the device or None -> clips [U,n] (written in place when given)."""
        geom = self._stream_geometry(rows, hop_samples, n_samples)
        if tuple(chunk.shape) != geom[:2]:
            raise L.EgError(f"audio shape {tuple(chunk.shape)} != ({geom[0]},{geom[1]})")
        if ends is not None and tuple(ends.shape) != (geom[0],):
            raise L.EgError(f"ends shape {tuple(ends.shape)} != ({geom[0]},)")
        if clips is not None and (tuple(clips.shape) != (geom[0], geom[2]) or clips.dtype != torch.float32 or not clips.is_contiguous()):
            raise L.EgError(f"clips: need a contiguous float32 [{geom[0]},{geom[2]}]")
        state = self._stream_state(state, geom)
        chunk = _need_cuda(chunk, "audio")
        ends = None if ends is None else _need_cuda(ends, "ends", torch.int32)
        if clips is None:
            clips = torch.empty(geom[0], geom[2], device=state.device)
        elif not clips.is_cuda:
            raise L.EgError("clips: the HIP path needs a GPU tensor; there is no CPU fallback")
        L.check(self._lib.eg_stream_push(self._h, _ptr(state), *geom, _ptr(chunk), _ptr(ends), _ptr(clips), _stream(state.device)), "eg_stream_push")
        return clips

    @_locked
    def stream_step(self, state, rows, hop_samples, n_samples, spec, text=None, sampled=None, alpha=None, want_window=False, want_prediction=False,
                    workspace=None):
        """eg_generator_stream_step: the generator at batch U seeded from the state's prior, then the stream's hand-off.  Returns a dict:
        rows [U,H,D], valid int32 [U], and window [U,F,D] / emotion_prediction [U,8] when wanted.  `workspace`: a private uint8 buffer of
        eg_generator_workspace_bytes(U) (a session that bakes it into a graph owns one); default: this engine's own."""
        geom = self._stream_geometry(rows, hop_samples, n_samples)
        U = geom[0]
        self._stream_step_args(U, spec, text, sampled, alpha)
        if self.arena is None:
            raise L.EgError("GeneratorEngine.stream_step before load_weights")
        state = self._stream_state(state, geom)
        dev = self.arena.device
        c = self.cfg
        spec = _need_cuda(spec, "spec")
        text = None if text is None else _need_cuda(text, "text", torch.int64)
        sampled = None if sampled is None else _need_cuda(sampled, "sampled")
        alpha = None if alpha is None else _need_cuda(alpha, "alpha")
        ws_bytes = self._lib.eg_generator_workspace_bytes(self._h, U)
        ws = self._workspace(("stream", U), ws_bytes, dev) if workspace is None else workspace
        if ws.numel() < ws_bytes or not ws.is_cuda:
            raise L.EgError(f"stream_step: workspace of {ws.numel()} bytes on {ws.device} (need {ws_bytes} on the GPU)")
        out = {"rows": torch.empty(U, c.frames - c.prior_frames, c.pose_dim, device=dev), "valid": torch.empty(U, dtype=torch.int32, device=dev)}
        if want_window:
            out["window"] = torch.empty(U, c.frames, c.pose_dim, device=dev)
        if want_prediction:
            out["emotion_prediction"] = torch.empty(U, 8, device=dev)
        L.check(self._lib.eg_generator_stream_step(
            self._h, _ptr(self.arena), _ptr(state), *geom, _ptr(spec), _ptr(text), _ptr(sampled), _ptr(alpha), _ptr(out["rows"]), _ptr(out["valid"]),
            _ptr(out.get("window")), _ptr(out.get("emotion_prediction")), _ptr(ws), ws_bytes, _stream(dev)), "eg_generator_stream_step")
        return out

    @_locked
    def stream_tail(self, state, rows, hop_samples, n_samples):
        """eg_stream_tail: the priors [U,P,D] = the last P rows of every row's track as it stands."""
        geom = self._stream_geometry(rows, hop_samples, n_samples)
        state = self._stream_state(state, geom)
        out = torch.empty(geom[0], self.cfg.prior_frames, self.cfg.pose_dim, device=state.device)
        L.check(self._lib.eg_stream_tail(self._h, _ptr(state), *geom, _ptr(out), _stream(state.device)), "eg_stream_tail")
        return out

    def tap(self, name: str, batch: int) -> torch.Tensor:
        """Copy of an intermediate of the last forward(batch) (parity tests)."""
        ws = self._ws[("fwd", batch)]
        p, n = C.c_void_p(), C.c_int64()
        L.check(self._lib.eg_generator_tap(self._h, batch, _ptr(ws), name.encode(), C.byref(p), C.byref(n)), "eg_generator_tap")
        off = p.value - ws.data_ptr()
        return ws[off: off + 4 * n.value].view(torch.float32).clone()


class CvaeEngine:
    """Host handle for eg_cvae_* (MLP_Reconstruct_v3, CAVE/BEAT_CVAE.py:312-460)."""

    def __init__(self, frames=60, d_model=512):
        lib = L.load()
        cfg = L.EgCvaeConfig()
        L.check(lib.eg_cvae_default_config(C.byref(cfg)), "eg_cvae_default_config")
        cfg.frames, cfg.d_model = frames, d_model
        self.cfg = cfg
        h = C.c_void_p()
        L.check(lib.eg_cvae_create(C.byref(cfg), C.byref(h)), "eg_cvae_create")
        self._h, self._lib = h, lib
        self.entries = packing.manifest(h, "eg_cvae_num_weights", "eg_cvae_weight_entry")
        self.arena_floats = lib.eg_cvae_arena_floats(h)
        self.arena = None
        self._ws = {}
        self._lock = threading.RLock()
        self.uploads = 0

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._lib.eg_cvae_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def load_weights(self, sd, device):
        with self._lock:
            self.arena = packing.build_arena(packing.strip_module_prefix(sd), self.entries, self.arena_floats).to(device)
            self._ws.clear()
            self.uploads += 1

    def _workspace(self, n, device, slot=0):
        nbytes = self._lib.eg_cvae_workspace_bytes(self._h, n)
        ws = self._ws.get((n, slot))                # one workspace per concurrent slot (ClipPipeline lane)
        if ws is None or ws.device != torch.device(device):
            ws = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
            self._ws[(n, slot)] = ws
        return ws, nbytes

    @_locked
    def sample(self, y, z, slot=0):
        dev = self.arena.device
        y, z = _need_cuda(y, "y"), _need_cuda(z, "z")
        n = y.shape[0]
        ws, nbytes = self._workspace(n, dev, slot)
        out = torch.empty(n, self.cfg.frames, self.cfg.d_model, device=dev)
        L.check(self._lib.eg_cvae_sample(self._h, _ptr(self.arena), n, _ptr(y), _ptr(z), _ptr(out), _ptr(ws), nbytes,
                                         _stream(dev)), "eg_cvae_sample")
        return out

    @_locked
    def forward(self, x, y, eps):
        dev = self.arena.device
        x, y, eps = _need_cuda(x, "x"), _need_cuda(y, "y"), _need_cuda(eps, "eps")
        n = x.shape[0]
        ws, nbytes = self._workspace(n, dev)
        rec = torch.empty(n, self.cfg.frames, self.cfg.d_model, device=dev)
        mu, logvar = torch.empty(n, 32, device=dev), torch.empty(n, 32, device=dev)
        L.check(self._lib.eg_cvae_forward(self._h, _ptr(self.arena), n, _ptr(x), _ptr(y), _ptr(eps), _ptr(rec), _ptr(mu),
                                          _ptr(logvar), _ptr(ws), nbytes, _stream(dev)), "eg_cvae_forward")
        return rec, mu, logvar


class MelFrontEnd:
    """extract_melspectrogram on the GPU (utils/train_utils_BEAT.py:186-190)."""

    def __init__(self, device):
        import numpy as np
        lib = L.load()
        fb, win, tw = np.zeros(513 * 128, np.float32), np.zeros(1024, np.float32), np.zeros(1024, np.float32)
        band = np.zeros(256, np.int32)
        L.check(lib.eg_mel_tables(host_ptr(fb), host_ptr(win), host_ptr(tw), host_ptr(band)), "eg_mel_tables")
        self.fb, self.win, self.tw, self.band = (torch.from_numpy(a).to(device) for a in (fb, win, tw, band))
        self._lib, self.device, self._ws, self._meta = lib, torch.device(device), {}, BoundedCache(64)

    def __call__(self, audio: torch.Tensor, out_frames: Optional[int] = None, slot: int = 0) -> torch.Tensor:
        audio = _need_cuda(audio, "audio")
        B, n = audio.shape
        n_frames = 1 + n // 512
        out_frames = n_frames if out_frames is None else out_frames
        nbytes = self._lib.eg_mel_workspace_bytes(B, n)
        ws = self._ws.get((B, n, slot))             # one workspace per concurrent slot (ClipPipeline lane)
        if ws is None:
            ws = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
            self._ws[(B, n, slot)] = ws
        spec = torch.empty(B, 128, out_frames, device=self.device)
        L.check(self._lib.eg_melspectrogram(_ptr(audio), B, n, _ptr(self.fb), _ptr(self.win), _ptr(self.tw), _ptr(self.band), _ptr(spec), out_frames,
                                            _ptr(ws), nbytes, _stream(self.device)), "eg_melspectrogram")
        return spec

    def windows(self, audio: torch.Tensor, windows: int, hop_samples: int, n_samples: int, out_frames: Optional[int] = None,
                slot: int = 0) -> torch.Tensor:
        """Long recordings [U, total_samples] -> spec [U, windows, 128, out_frames]: window w is the spectrogram of samples
        [w*hop_samples, w*hop_samples + n_samples) taken as a clip of its own, gathered on the device; a window that runs past the end is completed by symmetric padding
        of its own samples, as make_audio_fixed_length does."""
        audio = _need_cuda(audio, "audio")
        if audio.dim() != 2:
            raise L.EgError(f"audio shape {tuple(audio.shape)} != (U, total_samples)")
        if windows < 1 or hop_samples < 1:
            raise L.EgError(f"windows={windows} hop_samples={hop_samples} (need >= 1)")
        U, total = audio.shape
        clips = torch.empty(U * windows, n_samples, device=self.device)
        L.check(self._lib.eg_window_gather(_ptr(audio), U, total, windows, hop_samples, n_samples, _ptr(clips), _stream(self.device)),
                "eg_window_gather")
        spec = self(clips, out_frames, slot)
        return spec.view(U, windows, 128, spec.shape[-1])

    def windows_ragged(self, audio: torch.Tensor, lengths, hop_samples: int, n_samples: int, out_frames: Optional[int] = None, slot: int = 0):
        """Recordings of unequal length, audio [U, stride] with lengths[u] real samples each (what follows them is never read) -> (spec
        [N, 128, out_frames] packed recording-major, windows_per): recording u has W_u = ceil(lengths[u] / hop_samples) windows, every window
        that starts inside it; a window that runs past the recording's own end is completed by symmetric padding of its own samples."""
        if audio.dim() != 2:
            raise L.EgError(f"audio shape {tuple(audio.shape)} != (U, max_total_samples)")
        U, stride = int(audio.shape[0]), int(audio.shape[1])
        lens = int_list(lengths)
        if len(lens) != U:
            raise L.EgError(f"lengths: {len(lens)} entries for {U} recordings")
        if hop_samples < 1 or n_samples < 1:
            raise L.EgError(f"hop_samples={hop_samples} n_samples={n_samples} (need >= 1)")
        for u, v in enumerate(lens):
            if v < 1 or v > stride:
                raise L.EgError(f"lengths[{u}]={v} (need 1 .. {stride}, the width of audio)")
        audio = _need_cuda(audio, "audio")
        wp = [(v + hop_samples - 1) // hop_samples for v in lens]
        off = [sum(wp[:u]) for u in range(U)]
        meta = self._meta.get((tuple(lens), int(hop_samples)),   # lengths | offsets on the device, uploaded once per vector (the oldest goes first)
                              lambda: torch.tensor(lens + off, dtype=torch.int64).to(self.device))
        clips = torch.empty(sum(wp), n_samples, device=self.device)
        L.check(self._lib.eg_window_gather_ragged(_ptr(audio), U, stride, (C.c_int64 * U)(*lens), _ptr(meta), hop_samples, n_samples, _ptr(clips),
                                                  _stream(self.device)), "eg_window_gather_ragged")
        return self(clips, out_frames, slot), wp
