"""Streaming synthesis: gesture frames chunk by chunk from live audio.

`harness.synthesize` needs the whole recording; a `GestureStream` is the same roll-out fed one `hop` of audio at a time, for `rows`
speakers at once.  The session state -- an audio ring, the prior (the raw last `prior_frames` poses of the previous window) and per-row
counters -- lives on the device (include/emogest.h: eg_stream_*), and one step (push -> mel -> CVAE sample -> generator -> hand-off) is a
launch sequence that does not depend on the step index, so it is captured into ONE hipGraph and replayed for every step: window 0, the
steady state, the push in which a row ends and the steps after it differ only in device counters.

By definition a row's emitted rows, concatenated and followed by its `tail()`, are the `track` `harness.synthesize` returns for the same
audio `[:T]`, text, labels / z (or `sampled`), seed pose and `alpha`, with `windows` = the number of windows taken.

reset / push / ends are host-driven, so which rows are valid in a step is known on the host without reading the device: `SessionPlan` (built
on the pure functions `advance` / `plan`) mirrors the device counters.

No CPU fallback: everything here needs the HIP library and a GPU.
"""
from __future__ import annotations

import itertools
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib as L
from . import render as RD
from . import skeleton as SK
from . import smooth as SM
from ._host import int_list, need_cuda as _need_cuda
from .modules import _eval_only
from .pipeline import CAPTURE_MODE

__all__ = ["lag_of", "advance", "plan", "SessionPlan", "GestureStream", "AUTO_MEL"]

_SLOTS = itertools.count(1)
AUTO_MEL = object()         # `mel=AUTO_MEL` (the default of both open_stream entry points): a MelFrontEnd of the session's own on its device


# ---- the schedule, as pure functions of the per-row counters (c, w, total) ------------------------------------------------------------
def lag_of(hop: int, n: int) -> int:
    """Pushes a window spans: ceil(n / hop)."""
    return -(-int(n) // int(hop))


def advance(row: Tuple[int, int, int], hop: int, n: int, end: int = -1):
    """One push (and the step after it) for a row with counters `row = (c, w, total)`: c pushes since its reset, w windows done, total = -1
    while it is open, else the samples it was fed.  `end = m in [0, hop]`: the row ends in this push, only its first m samples are real.
    Returns (new row, info): info["valid"], and for a valid step "w" (the window emitted), "offset" (its start in the ring, counted from the
    oldest sample held) and "L" (its real samples; < n: completed by symmetric padding of its own samples)."""
    c, w, total = row
    lag = lag_of(hop, n)
    c += 1
    if total < 0 and end is not None and end >= 0:
        total = (c - 1) * hop + min(int(end), hop)
    valid = c >= w + lag if total < 0 else w * hop < total
    info = {"valid": bool(valid), "w": None, "offset": None, "L": None}
    if valid:
        info.update(w=w, offset=(w + lag - c) * hop, L=n if total < 0 else min(n, total - w * hop))
        w += 1
    return (c, w, total), info


def plan(hop: int, n: int, total_samples: int, steps: int) -> List[dict]:
    """The schedule of one row for a recording of `total_samples` samples fed hop by hop (the push that holds its last sample ends it,
    later pushes carry nothing) over `steps` pushes: the `info` of `advance` per step."""
    last = max(1, -(-int(total_samples) // hop))
    row, out = (0, 0, -1), []
    for s in range(1, steps + 1):
        row, info = advance(row, hop, n, total_samples - (last - 1) * hop if s == last else -1)
        out.append(info)
    return out


class SessionPlan:
    """Host mirror of a session's device counters.  `coupled`: the memory variant, whose TM_Memory_Net mixes the rows of a step, so only
    whole-session reset / end is accepted there (every row valid together: the result is the roll-out's)."""
    _WHY = ("the memory variant's TM_Memory_Net couples the rows of a step, so a row's poses depend on every other row's prior: "
            "only a whole-session reset / end is accepted (rows of the spatial variant are independent)")

    def __init__(self, rows: int, hop: int, n: int, coupled: bool = False):
        if rows < 1 or hop < 1 or n < 1:
            raise L.EgError(f"stream: rows={rows} hop_samples={hop} n_samples={n} (need >= 1)")
        self.U, self.hop, self.n, self.coupled = int(rows), int(hop), int(n), bool(coupled)
        self.rows = [(0, 0, -1)] * self.U
        self.finished = False

    def _ends(self, ends) -> List[int]:
        if ends is None:
            return [-1] * self.U
        if isinstance(ends, int):
            ends = [ends] * self.U
        ends = int_list(ends)
        if len(ends) != self.U:
            raise L.EgError(f"ends: {len(ends)} values for {self.U} rows")
        if any(e < -1 or e > self.hop for e in ends):
            raise L.EgError(f"ends: every value must be -1 (the row goes on) or in [0, {self.hop}] (got {ends})")
        return ends

    def check_open(self) -> None:
        if self.finished:
            raise L.EgError("push after finish: the session has ended (reset() opens it again)")

    def preview(self, ends=None):
        """(new rows, infos) of a push, nothing committed; refuses what the variant cannot do."""
        self.check_open()
        ends = self._ends(ends)
        new = [advance(r, self.hop, self.n, e) for r, e in zip(self.rows, ends)]
        if self.coupled:
            if len({r[2] >= 0 for r, _i in new}) > 1:
                raise L.EgError("ends for a subset of the rows: " + self._WHY)
            if len({-(-r[2] // self.hop) for r, _i in new if r[2] >= 0}) > 1:       # e.g. ends = 0 beside ends > 0: one window fewer
                raise L.EgError(f"ends {ends}: the rows would end with different numbers of windows: " + self._WHY)
            if len({i["valid"] for _r, i in new}) > 1:
                raise L.EgError("rows out of step (a row valid where another is not): " + self._WHY)
        return [r for r, _i in new], [i for _r, i in new], ends

    def push(self, ends=None) -> List[dict]:
        rows, infos, _e = self.preview(ends)
        self.rows = rows
        return infos

    def remaining(self, ends=None) -> List[int]:
        """Windows every row can still emit if the session ended with this push (`ends`; None: 0 real samples in it)."""
        ends = self._ends(0 if ends is None else ends)
        out = []
        for (c, w, total), e in zip(self.rows, ends):
            if total < 0:
                total = c * self.hop + (min(e, self.hop) if e >= 0 else self.hop)
            out.append(max(0, -(-total // self.hop) - w))
        return out

    def reset(self, rows: Optional[Sequence[int]] = None) -> List[int]:
        sel = list(range(self.U)) if rows is None else sorted({int(r) for r in rows})
        if any(r < 0 or r >= self.U for r in sel) or not sel:
            raise L.EgError(f"reset: rows {sel} of a session of {self.U}")
        if self.coupled and len(sel) != self.U:
            raise L.EgError("reset of a subset of the rows: " + self._WHY)
        for r in sel:
            self.rows[r] = (0, 0, -1)
        self.finished = False
        return sel


# ---- the session -----------------------------------------------------------------------------------------------------------------------
class GestureStream:
    """`models = (generator, vae | None, mel | None)`: modules on the GPU, eval mode.  `rows` = U speakers; `seed_pose [U, P, D]`.

    With a mel front-end: `push(audio [U, hop], text [U, text_len], labels [U, 8] (+ z [U, 32]) | sampled [U, F, d_model], ends=None)`
    -> `(rows [U, H, D] | None, valid int32 [U])`; every push advances every row by one hop.  A row whose window is not ready (its first
    `lag - 1` pushes, or ended and out of windows) is not valid in that step: zero rows, prior unchanged.  While no row is valid only the
    push kernels run and `rows` is None.  `ends[u] = m in [0, hop]` (host values: int, list or CPU tensor) ends row u in this push: only
    its first m samples are real.  `mel=None`: `push_spec(spec [U, n_mels, spec_len], text, ...)`, one ready window per call.
    `hop_samples` / `n_samples` default to the generator's geometry as in harness.synthesize; `graph=True` replays one captured hipGraph.
    `joints=skeleton` (a skeleton.Skeleton with 3K == pose_dim; `joints_mean [pose_dim]`, `joints_unit` as in skeleton.joints_from_tracks): every
    step ends with one more launch (inside the graph) that leaves the joint positions of the rows just emitted in `last_joints [U, H, J, 3]`
    -- zeros for a row that was not valid, None while `rows` is None; `push` returns what it returned.  `tail_joints()`: the joints of `tail()`.
    `joints_fps` is refused: a frame-rate change needs the frame after the last one emitted.
    `rotations=rest` (with `joints=`; `rest [K, 3]` the avatar's bind pose, `rotations_space` as in skeleton.rotations_from_tracks): one more
    launch inside the graph leaves the bone rotations of the rows just emitted in `last_rotations [U, H, K, 4]` under the same rules;
    `tail_rotations()`: the rotations of `tail()`.
    `joints=tree` (a skeleton.JointTree with 6J == pose_dim: the BEAT generators' 6-D joint rotations; `rotations=True` for the rotations too):
    ONE more launch inside the graph fills `last_joints [U, H, J, 3]` and `last_rotations [U, H, J, 4]` under the same rules, and
    `tail_joints()` / `tail_rotations()` work likewise; `joints_unit` and a rest pose are refused by name.
    `euler=order | BvhFile` (with `joints=tree`; as in harness.synthesize): one more launch inside the graph leaves the BVH rotation channels of
    the rows just emitted in `last_euler [U, H, J, 3]` (degrees, principal values) under the same rules; `tail_euler()`: those of `tail()`.  A
    row's `last_euler` followed by its `tail_euler()` are skeleton.euler_from_rot6d on its finished track bit for bit.  `euler_unwrap=True` is
    refused by name: unwrap the finished track (skeleton.unwrap_angles).
    `smooth=Smoother | (window, polyorder)` (smooth.Smoother, deriv 0, window <= H): every step ends with the two launches of a
    smooth.StreamSmoother (inside the graph) that leave in `last_smooth [U, H, D]` the smoothed frames `[sH - half, (s + 1)H - half)` of a row in
    its s-th valid step -- `smooth_delay = half` frames behind the rows just emitted, the first `half` entries of step 0 zeros; zeros for a row
    that was not valid, None while `rows` is None.  `tail_smooth()`: the last `[U, P + half, D]` smoothed frames.  A row's `last_smooth`,
    concatenated after dropping step 0's leading `half` entries, followed by `tail_smooth()`, is smooth.smooth_tracks on its finished track bit
    for bit.  `reset(rows=)` resets the smoothing state of those rows.  Not together with `joints=`: the first `half` entries of step 0 are not
    poses.
    `render=RenderSpec | dict` (render.RenderSpec: `joints`, `mean`, `unit`, `fps=(src, dst)`, `rotations`, `rotations_space`, `euler`, `smooth`):
    the delayed output stage, independent of the arguments above -- what `smooth=` with `joints=` and `joints_fps=` refuse.  Every step ends
    with the launches of a render.StreamRender (inside the graph) that leave in `last_render = {name: [U, render_frames, ., .]}` the smoothed
    joints / rotations / Euler channels at the output rate, `render_delay` source frames behind the rows just emitted (`render_delay / fps`
    seconds); the first `render_lead` entries of a row's first valid step are zeros, a row that was not valid has zeros, None while `rows` is
    None.  `tail_render()`: the last output frames.  For every name a row's `last_render`, concatenated after dropping the first step's
    leading `render_lead` entries, followed by `tail_render()`, is `harness.synthesize(smooth=, joints=, rotations=, euler=, joints_fps=)` on
    its finished track bit for bit."""

    def __init__(self, models: Tuple, rows: int, seed_pose: torch.Tensor, *, hop_samples: Optional[int] = None, n_samples: Optional[int] = None,
                 fps: int = 15, sample_rate: int = 16000, alpha: Optional[torch.Tensor] = None, graph: bool = True, want_windows: bool = False,
                 draws: Optional[int] = None, audio_rate: Optional[int] = None, joints=None, joints_mean=None, joints_unit: bool = False,
                 joints_fps=None, rotations=None, rotations_space: str = "local", smooth=None, euler=None, euler_unwrap: bool = False,
                 render=None):
        # the output stage: what needs no model is checked here, the rest once pose_dim is known
        outputs = SK.TrackOutputs("GestureStream", joints, joints_mean, joints_unit, joints_fps, rotations, rotations_space, euler, euler_unwrap,
                                  streaming=True)
        if smooth is not None:
            if joints is not None:
                raise L.EgError("GestureStream: smooth= together with joints= is not supported (the smoothed rows run half a window behind and "
                                "the first `half` entries of step 0 are not poses); take joints from the raw rows, or smooth the finished "
                                "track with harness.synthesize(..., smooth=, joints=); in a live session: render=")
            smooth = SM.Smoother.of(smooth, "GestureStream: smooth", fps)
        render = None if render is None else RD.RenderSpec.of(render)          # refuses what needs no model
        if draws is not None:
            raise L.EgError("GestureStream: draws= is not supported (a stream has one track per row); for several sampled tracks of a whole "
                            "recording call the rectangular synthesize(..., draws=R), or open the stream with each speaker's row repeated")
        self.gen, self.vae, self.mel = models
        if self.mel is None and (hop_samples is not None or n_samples is not None):
            raise L.EgError("hop_samples / n_samples: the session has no mel front-end (models[2] is None); it takes one ready window per push_spec")
        _eval_only(self.gen)
        if self.vae is not None:
            _eval_only(self.vae)
        c = self.gen._cfg
        self.F, self.P, self.D, self.d_model = c["frames"], c["prior_frames"], c["pose_dim"], c["d_model"]
        self.H = self.F - self.P
        self.text_len, self.n_mels, self.spec_len = c["text_len"], c["n_mels"], c["spec_len"]
        self.U = int(rows)
        # it holds the mean, the tables and the order codes on the device: the captured graph replays their addresses
        self._outs: Optional[SK.TrackOutputs] = outputs.fit(self.D)
        if self.mel is not None:
            self.hop = int(round(self.H * sample_rate / fps)) if hop_samples is None else int(hop_samples)
            self.n = (self.spec_len - 1) * 512 if n_samples is None else int(n_samples)
        else:                   # ready spectrograms: one window per push; the ring degenerates to one sample per row
            self.hop = self.n = 1
        # audio at another rate: a StreamResampler in front of the ring (its two launches come first in every step, inside the captured graph)
        self.audio_rate = None if audio_rate is None or int(audio_rate) == int(sample_rate) else int(audio_rate)
        self.hop_in, self._rs, self._ratio = self.hop, None, (1, 1)
        if self.audio_rate is not None:
            from . import resample as RS
            if self.mel is None:
                raise L.EgError("GestureStream: audio_rate= with a session that has no mel front-end (models[2] is None): push_spec takes ready "
                                "spectrograms, there is no audio to resample")
            self._ratio = RS.ratio(self.audio_rate, sample_rate)                # refuses an unsupported ratio by name
            if self.hop * self._ratio[1] % self._ratio[0]:
                raise L.EgError(RS.hop_message("GestureStream", self.hop, self.audio_rate, sample_rate))
            self.hop_in = self.hop * self._ratio[1] // self._ratio[0]
        self.plan = SessionPlan(self.U, self.hop, self.n, coupled=c["variant"] == "memory")
        self.lag = lag_of(self.hop, self.n)
        if tuple(seed_pose.shape) != (self.U, self.P, self.D):
            raise L.EgError(f"seed_pose shape {tuple(seed_pose.shape)} != ({self.U},{self.P},{self.D})")
        if alpha is not None and tuple(alpha.shape) != (self.P,):
            raise L.EgError(f"alpha shape {tuple(alpha.shape)} != ({self.P},)")
        self.seed_pose = _need_cuda(seed_pose, "seed_pose").clone()
        self.alpha = None if alpha is None else _need_cuda(alpha, "alpha").clone()
        self.device = self.seed_pose.device
        if self._outs is not None:
            self._outs.to(self.device)
        if self.mel is AUTO_MEL:
            from .engine import MelFrontEnd
            self.mel = MelFrontEnd(self.device)
        self.use_graph, self.want_windows = bool(graph), bool(want_windows)
        self._slot = ("stream", next(_SLOTS))        # private mel / CVAE workspaces
        eng = self._engine()
        self._geom = (self.U, self.hop, self.n)
        dev = self.device
        self._state = torch.zeros(eng.stream_state_bytes(*self._geom), dtype=torch.uint8, device=dev)
        self._ws = torch.empty(int(eng._lib.eg_generator_workspace_bytes(eng._h, self.U)), dtype=torch.uint8, device=dev)
        z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device=dev)
        self._in: Dict[str, torch.Tensor] = {"audio": z(self.U, self.hop), "ends": torch.full((self.U,), -1, dtype=torch.int32, device=dev),
                                             "text": z(self.U, self.text_len, dtype=torch.int64)}
        if self.audio_rate is not None:
            from .resample import StreamResampler
            self._rs = StreamResampler(self.U, self.audio_rate, self.hop, sample_rate, device=dev)
            self._in["audio"] = self._rs.out                         # the ring is fed the resampler's static output
        self._clips = z(self.U, self.n)
        if self.mel is None:
            self._in["spec"] = z(self.U, self.n_mels, self.spec_len)
        if self.vae is not None:
            self._in["label"], self._in["z"] = z(self.U, 8), z(self.U, 32)
        # the smoother's state, table and output are held here: the captured graph replays their addresses
        self._sm = None if smooth is None else SM.StreamSmoother(self.U, self.H, self.D, smooth, device=dev)
        self.smooth_delay: Optional[int] = None if self._sm is None else self._sm.delay
        # the delayed output stage, with a smoother, a delay line and outputs of its own: static buffers, as above
        self._rd = None if render is None else RD.StreamRender(self.U, self.H, self.P, self.D, render, device=dev, src_fps=fps)
        self.render_delay, self.render_frames, self.render_lead = (None,) * 3 if self._rd is None else (self._rd.delay, self._rd.frames, self._rd.lead)
        self._graphs: Dict[bool, dict] = {}
        self.last_valid: List[bool] = [False] * self.U           # the host's verdict for the last step, and the window index per valid row
        self.last_windows: List[Optional[int]] = [None] * self.U
        self.last_window: Optional[torch.Tensor] = None          # with want_windows: the raw poses [U, F, D] of the last step
        self.last_joints: Optional[torch.Tensor] = None          # with joints=: the joints [U, H, J, 3] of the rows just emitted (zeros for a row that was not valid)
        self.last_rotations: Optional[torch.Tensor] = None       # with rotations=: their bone rotations [U, H, K, 4], under the same rules
        self.last_euler: Optional[torch.Tensor] = None           # with euler=: their Euler channels [U, H, J, 3] in degrees (principal values), likewise
        self.last_smooth: Optional[torch.Tensor] = None          # with smooth=: the smoothed frames [U, H, D], smooth_delay frames behind the rows
        self.last_render: Optional[Dict[str, torch.Tensor]] = None       # with render=: {name: [U, render_frames, ., .]}, render_delay frames behind the rows
        eng.stream_reset(self._state, *self._geom, self.seed_pose)

    # ---- engines, staleness ----
    def _engine(self):
        _eval_only(self.gen)
        return self.gen.engine()

    def _engine_state(self):
        eng = self._engine()
        veng = self.vae.engine() if self.vae is not None else None
        return eng, eng.arena, veng, (veng.arena if veng is not None else None)

    def stale(self) -> bool:
        """True when a captured graph points at engines / weight arenas that are no longer the models' (weights reloaded, precision changed)."""
        key = tuple(id(o) for o in self._engine_state())
        return any(g["key"] != key for g in self._graphs.values())

    def refresh(self) -> None:
        """Re-capture against the models' current engines; counters, ring and prior are kept."""
        torch.cuda.synchronize(self.device)
        for k in list(self._graphs):
            self._graphs[k] = self._capture(k)

    def _own(self, ws: Optional[dict]) -> Optional[dict]:
        """This session's entries of an engine's workspace table (keys end in the slot)."""
        return None if ws is None else {k: v for k, v in ws.items() if k[-1] == self._slot}

    def close(self) -> None:
        """Drop the graphs and the session's private mel / CVAE workspaces."""
        self._graphs.clear()
        veng = self.vae._engine if self.vae is not None else None
        for ws in (self.mel._ws if self.mel is not None and self.mel is not AUTO_MEL else None, veng._ws if veng is not None else None):
            for k in list(self._own(ws) or ()):
                ws.pop(k, None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- one step on the current stream, reading the static buffers ----
    def _run_step(self, use_sampled: bool):
        g = self._in
        with torch.no_grad():
            eng = self._engine()
            clips = self._push_only()
            spec = self.mel(clips, out_frames=self.spec_len, slot=self._slot) if self.mel is not None else g["spec"]
            if self.vae is not None:
                sampled = self.vae.sample(g["label"], z=g["z"], slot=self._slot)
            else:
                sampled = g["sampled"] if use_sampled else None
            out = eng.stream_step(self._state, *self._geom, spec, g["text"], sampled, self.alpha, want_window=self.want_windows,
                                  workspace=self._ws)
            if self._outs is not None:              # the outputs of the rows just emitted, after the hand-off: row u has valid[u] * H frames
                out.update(self._outs.launch(out["rows"], out["valid"], 1, self.H))
            if self._sm is not None:                # the outputs, then the new history in a launch of its own
                out["smooth"] = self._sm.run(out["rows"], out["valid"])
            if self._rd is not None:                # the delayed stage: its smoother, its delay line, then the output launches
                out["render"] = self._rd.run(out["rows"], out["valid"])
            return out

    def _push_only(self):
        """The resampler's launches (with audio_rate), then the ring's: the part of a step that runs even when no row has a window."""
        if self._rs is not None:
            self._rs.run()
        return self._engine().stream_push(self._state, *self._geom, self._in["audio"], self._in["ends"], self._clips)

    def _capture(self, use_sampled: bool) -> dict:
        """Two eager warm-up runs on a side stream (workspaces, kernel attributes: outside the capture), then the capture; the session's state is
        snapshotted before and restored after, so neither advances it."""
        dev = self.device
        snap = self._state.clone()
        rs_snap = self._rs.snapshot() if self._rs is not None else None      # the resampler's history advances with every run, too
        sm_snap = self._sm.snapshot() if self._sm is not None else None      # and the smoother's
        rd_snap = self._rd.snapshot() if self._rd is not None else None      # and the render stage's
        cap = torch.cuda.Stream(dev)
        cap.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(cap):
            for _ in range(2):
                self._run_step(use_sampled)
        torch.cuda.current_stream(dev).wait_stream(cap)
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode=CAPTURE_MODE):
            out = self._run_step(use_sampled)
        self._state.copy_(snap)
        if self._rs is not None:
            self._rs.restore(rs_snap)
        if self._sm is not None:
            self._sm.restore(sm_snap)
        if self._rd is not None:
            self._rd.restore(rd_snap)
        torch.cuda.synchronize(dev)
        # the graph replays raw pointers into the engines' arenas and workspaces: keep them alive as long as the graph (ClipPipeline._capture)
        st = self._engine_state()
        keep = st + (self._own(st[2]._ws if st[2] is not None else None), self._own(self.mel._ws if self.mel is not None else None))
        return {"graph": graph, "out": out, "key": tuple(id(o) for o in st), "keep": keep}

    def _launch(self, use_sampled: bool) -> dict:
        if not self.use_graph:
            return self._run_step(use_sampled)
        g = self._graphs.get(use_sampled)
        if g is None:
            g = self._graphs[use_sampled] = self._capture(use_sampled)
        g["graph"].replay()
        return g["out"]

    _STALE = ("GestureStream: the models' engine / weight arena changed after capture (weights reloaded or precision flipped); "
              "call refresh() before the next push (the session's state is kept)")

    def _check_fresh(self) -> None:
        """Before a push commits anything: a stale graph is refused, as ClipPipeline.launch_next refuses one."""
        if self.use_graph and self._graphs and self.stale():
            raise RuntimeError(self._STALE)

    def replay(self, use_sampled: bool = False) -> dict:
        """Low level (the bench drives this): replay the captured step on the static buffers as they stand; returns the graph's own output
        tensors.  Staleness is checked by identity only, without packing anything.  EVERY REPLAY ADVANCES THE DEVICE COUNTERS BY ONE PUSH AND THE
        HOST PLAN BY NONE: after it the session's `push` / `last_valid` are off by the replays made, so a session driven this way is for timing
        only (reset() brings both back in step)."""
        g = self._graphs.get(use_sampled)
        if g is not None:
            eng = self.gen.engine_peek()
            if eng is None or id(eng) != g["key"][0] or id(eng.arena) != g["key"][1]:
                raise RuntimeError(self._STALE)
        return self._launch(use_sampled)

    # ---- the public surface ----
    def _fill(self, name: str, src: Optional[torch.Tensor], shape, dtype=torch.float32) -> None:
        buf = self._in.get(name)
        if buf is None:
            buf = self._in[name] = torch.zeros(*shape, dtype=dtype, device=self.device)
        buf.copy_(src, non_blocking=True)

    def _conditioning(self, labels, z, sampled):
        """Checks the emotion inputs; returns use_sampled."""
        if self.vae is not None:
            if labels is None:
                raise L.EgError(f"labels: needed when a VAE is given ([{self.U}, 8] one-hot)")
            if tuple(labels.shape) != (self.U, 8):
                raise L.EgError(f"labels shape {tuple(labels.shape)} != ({self.U},8)")
            if z is not None and tuple(z.shape) != (self.U, 32):
                raise L.EgError(f"z shape {tuple(z.shape)} != ({self.U},32)")
            if sampled is not None:
                raise L.EgError("sampled: the session has a VAE, which makes the emotion feature from labels / z")
            _need_cuda(labels, "labels")
            return False
        if sampled is not None:
            if tuple(sampled.shape) != (self.U, self.F, self.d_model):
                raise L.EgError(f"sampled shape {tuple(sampled.shape)} != ({self.U},{self.F},{self.d_model})")
            _need_cuda(sampled, "sampled")
            return True
        return False

    def _step(self, audio, spec, text, labels, z, sampled, ends):
        self.plan.check_open()
        if tuple(text.shape) != (self.U, self.text_len):
            raise L.EgError(f"text shape {tuple(text.shape)} != ({self.U},{self.text_len})")
        use_sampled = self._conditioning(labels, z, sampled)
        _need_cuda(text, "text", torch.int64)
        ends_in = None
        if self._rs is not None:
            ends, ends_in = self._ends_at_model_rate(ends)
        rows, infos, ends_host = self.plan.preview(ends)            # refuses before anything touches the device
        self._check_fresh()
        if audio is not None and self._rs is not None:
            self._rs.chunk.copy_(audio, non_blocking=True)
            self._rs.ends.copy_(torch.tensor(ends_in, dtype=torch.int32), non_blocking=False)
        elif audio is not None:
            self._in["audio"].copy_(audio, non_blocking=True)
        if spec is not None:
            self._in["spec"].copy_(spec, non_blocking=True)
        self._in["ends"].copy_(torch.tensor(ends_host, dtype=torch.int32), non_blocking=False)
        self._in["text"].copy_(text, non_blocking=True)
        if self.vae is not None:
            self._in["label"].copy_(labels, non_blocking=True)
            self._in["z"].copy_(torch.randn(self.U, 32) if z is None else z)        # the CPU generator, as MLP_Reconstruct_v3.sample draws
        elif use_sampled:
            self._fill("sampled", sampled, (self.U, self.F, self.d_model))
        valid = [i["valid"] for i in infos]
        if any(valid):
            out = self._launch(use_sampled)
        else:
            out = None
            with torch.no_grad():
                self._push_only()
        # the host mirror follows the device: committed once the push has been enqueued (a launch or capture that raises leaves both where they were)
        self.plan.rows, self.last_valid, self.last_windows = rows, valid, [i["w"] for i in infos]
        self.last_window = out["window"].clone() if out is not None and self.want_windows else None
        self.last_joints, self.last_rotations, self.last_euler = (out[name].clone() if out is not None and name in out else None
                                                                  for name in ("joints", "rotations", "euler"))
        self.last_smooth = out["smooth"].clone() if out is not None and self._sm is not None else None
        self.last_render = {n: v.clone() for n, v in out["render"].items()} if out is not None and self._rd is not None else None
        if out is None:
            return None, torch.zeros(self.U, dtype=torch.int32, device=self.device)
        return out["rows"].clone(), out["valid"].clone()

    def _ends_at_model_rate(self, ends):
        """With audio_rate: `ends` counts input samples, [0, hop_in].  -> (the same ends in model-rate samples for the session's plan and ring,
        the resampler's vector: a row that ended in an earlier push carries nothing, 0 real samples)."""
        e_in = self._rs.host_ends(ends)
        Lf, M = self._ratio
        e_out = [-1 if m < 0 else -(-m * Lf // M) for m in e_in]
        e_rs = [0 if row[2] >= 0 else m for row, m in zip(self.plan.rows, e_in)]
        return e_out, e_rs

    def push(self, audio, text, labels=None, z=None, sampled=None, ends=None):
        if self.mel is None:
            raise L.EgError("push: the session has no mel front-end (models[2] is None); feed ready spectrograms with push_spec")
        if tuple(audio.shape) != (self.U, self.hop_in):
            raise L.EgError(f"audio shape {tuple(audio.shape)} != ({self.U},{self.hop_in})" +
                            (f" ({self.hop} samples per push at the model's rate are {self.hop_in} at audio_rate={self.audio_rate})"
                             if self._rs is not None else ""))
        _need_cuda(audio, "audio")
        return self._step(audio, None, text, labels, z, sampled, ends)

    def push_spec(self, spec, text, labels=None, z=None, sampled=None, ends=None):
        """`mel=None` sessions: one ready window per call (ClipPipeline's convention for ready spectrograms).  `ends[u] = 1`: this is row
        u's last window; `0`: the row ended before it (this call carries nothing for it)."""
        if self.mel is not None:
            raise L.EgError("push_spec: the session has a mel front-end; feed audio with push")
        if tuple(spec.shape) != (self.U, self.n_mels, self.spec_len):
            raise L.EgError(f"spec shape {tuple(spec.shape)} != ({self.U},{self.n_mels},{self.spec_len})")
        _need_cuda(spec, "spec")
        return self._step(None, spec, text, labels, z, sampled, ends)

    def reset(self, rows: Optional[Sequence[int]] = None, seed_pose: Optional[torch.Tensor] = None) -> None:
        """Rows `rows` (None: all) start a new recording: counters to zero, ring zeroed, prior := seed_pose[row] (`seed_pose [U, P, D]`,
        default the construction's).  A subset is refused on the memory variant."""
        seed = self.seed_pose if seed_pose is None else seed_pose
        if tuple(seed.shape) != (self.U, self.P, self.D):
            raise L.EgError(f"seed_pose shape {tuple(seed.shape)} != ({self.U},{self.P},{self.D})")
        seed = _need_cuda(seed, "seed_pose")
        sel = self.plan.reset(rows)
        mask = None
        if len(sel) != self.U:
            m = torch.zeros(self.U, dtype=torch.int32)
            m[sel] = 1
            mask = m.to(self.device)
        self._engine().stream_reset(self._state, *self._geom, seed, mask)
        if self._rs is not None:
            self._rs.reset(None if len(sel) == self.U else sel)
        if self._sm is not None:
            self._sm.reset(None if len(sel) == self.U else sel)
        if self._rd is not None:
            self._rd.reset(None if len(sel) == self.U else sel)

    def tail(self) -> torch.Tensor:
        """[U, P, D]: every row's current prior = the last P rows of its track."""
        return self._engine().stream_tail(self._state, *self._geom)

    def tail_joints(self) -> torch.Tensor:
        """[U, P, J, 3]: the joints of `tail()` (a session opened with joints=)."""
        return self._tail_output("joints", "joints=skeleton")

    def tail_rotations(self) -> torch.Tensor:
        """[U, P, K, 4]: the bone rotations of `tail()` (a session opened with rotations=)."""
        return self._tail_output("rotations", "rotations=rest")

    def tail_euler(self) -> torch.Tensor:
        """[U, P, J, 3]: the Euler channels of `tail()` in degrees (a session opened with euler=)."""
        return self._tail_output("euler", "euler=order")

    def _tail_output(self, name: str, opened_with: str) -> torch.Tensor:
        if self._outs is None or name not in self._outs.made:
            raise L.EgError(f"tail_{name}: the session was opened without {opened_with}")
        with torch.no_grad():
            return self._outs.launch(self.tail(), want=(name,))[name]

    def tail_smooth(self) -> torch.Tensor:
        """[U, P + smooth_delay, D]: the last smoothed frames of every row's track (a session opened with smooth=); zeros for a row that has
        emitted nothing."""
        if self._sm is None:
            raise L.EgError("tail_smooth: the session was opened without smooth=")
        with torch.no_grad():
            return self._sm.tail(self.tail())

    def tail_render(self) -> Dict[str, torch.Tensor]:
        """{name: [U, n_tail, ., .]}: the last output frames of every row's track (a session opened with render=); zeros for a row that has
        emitted nothing."""
        if self._rd is None:
            raise L.EgError("tail_render: the session was opened without render=")
        with torch.no_grad():
            return self._rd.tail(self.tail())

    def finish(self, text, labels=None, z=None, sampled=None, last_chunk=None, ends=None) -> torch.Tensor:
        """End every row together and run R = text.shape[1] steps in all: `text [U, R, text_len]`, `labels [U, 8]` or `[U, R, 8]`, `z [U, R, 32]`
        | `sampled [U, R, F, d_model]`.  `last_chunk [U, hop]` with `ends` (default hop: all of it real) when the recording stops inside a hop;
        without it the recording stopped with the last push.  R is at most the windows that remain for the row that has most.  Returns the
        rows of those steps with the tail appended, `[U, R*H + P, D]` (a row that runs out of windows earlier has zero rows from there on)."""
        if self.mel is None:
            raise L.EgError("finish: needs a mel front-end; with ready spectrograms end rows with push_spec(..., ends=...) and read tail()")
        self.plan.check_open()
        if text.dim() != 3 or tuple(text.shape[::2]) != (self.U, self.text_len) or text.shape[1] < 1:
            raise L.EgError(f"text shape {tuple(text.shape)} != ({self.U},R,{self.text_len})")
        R = int(text.shape[1])
        if last_chunk is None:
            if ends is not None:
                raise L.EgError("finish: ends without last_chunk")
            ends, chunk = 0, torch.zeros(self.U, self.hop_in, device=self.device)
        else:
            ends, chunk = self.hop_in if ends is None else ends, last_chunk
        left = max(self.plan.remaining(self._ends_at_model_rate(ends)[0] if self._rs is not None else ends))
        if R > left:
            raise L.EgError(f"finish: R={R} steps asked, {left} windows remain")
        lab = lambda r: None if labels is None else (labels[:, r] if labels.dim() == 3 else labels)
        out = []
        for r in range(R):
            rows, _valid = self.push(chunk if r == 0 else torch.zeros_like(chunk), text[:, r], lab(r), None if z is None else z[:, r],
                                     None if sampled is None else sampled[:, r], ends=ends if r == 0 else None)
            out.append(torch.zeros(self.U, self.H, self.D, device=self.device) if rows is None else rows)
        self.plan.finished = True
        return torch.cat(out + [self.tail()], 1)
