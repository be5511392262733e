"""Preview frames on the GPU (eg_preview_raster through preview.render_joints, harness.synthesize(preview=) and synthesize_takes(preview=)):
every comparison is exact equality of the uint8 pictures with the numpy float32 restatement tests/preview_np.py.  The cases, and the check
that the restatement's own pictures are not blank, are tests/preview_cases.py's."""
import numpy as np
import pytest
import torch

import preview_cases as PC
from emotiongestures_amd import _lib as L
from emotiongestures_amd import harness as Hs
from emotiongestures_amd import preview as PV
from emotiongestures_amd import skeleton as SK
from emotiongestures_amd.synth import synth_audio
from skeleton_gpu_common import H_, HOP, N, P_, dev, inputs, ted_models

pytestmark = pytest.mark.gpu


def mismatch(got, want):
    """'' when equal; else where the first differing bytes are."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    if got.shape != want.shape:
        return f"shape {got.shape} != {want.shape}"
    bad = np.argwhere(got != want)
    return "" if not len(bad) else f"{len(bad)} of {want.size} bytes differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


@pytest.mark.parametrize("name", PC.NAMES)
def test_kernel_equals_the_restatement_byte_for_byte(name):
    joints, frames, spec, want = PC.case(name)
    got = PV.render_joints(torch.from_numpy(joints).to(dev()), spec, frames)
    assert got.is_cuda and got.dtype == torch.uint8
    assert not mismatch(got, want)
    if frames is not None:                                                               # frames 4-6 of recording 1 are zeros
        assert not got[1, :, frames[1]:].any() and got[1, :, :frames[1]].any()


def test_a_slice_that_starts_off_a_16_byte_boundary_and_one_row_of_many():
    """A view into a larger tensor goes through the front end's aligned copy; a row's pictures do not depend on the batch."""
    joints, frames, spec, want = PC.case("ted-hwc-rgb")
    flat = torch.zeros(joints.size + 1, dtype=torch.float32, device=dev())
    flat[1:] = torch.from_numpy(joints).to(dev()).reshape(-1)
    assert not mismatch(PV.render_joints(flat[1:].reshape(joints.shape), spec, frames), want)
    one = PV.render_joints(torch.from_numpy(joints[0, 1]).to(dev()), spec)
    assert not mismatch(one, want[0, 1])


def test_graph_replay_equals_the_eager_call():
    from emotiongestures_amd.pipeline import CAPTURE_MODE
    joints, _frames, spec, want = PC.case("clipped")
    rows = torch.from_numpy(joints[None]).to(dev())                                      # [1, 2, 43, 3]
    d_frames = torch.tensor([2], dtype=torch.int32, device=dev())
    PV.launch_preview(rows, spec, d_frames)                                              # the warm-up: the table is uploaded here
    out = torch.full((1, 2) + spec.frame_shape(), 7, dtype=torch.uint8, device=dev())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode=CAPTURE_MODE):
        PV.launch_preview(rows, spec, d_frames, out=out)
    shifted = joints[None] + np.float32(0.05)
    for k, (src, n) in enumerate(((joints[None], 2), (shifted, 1))):                     # new joints and a new count: the graph reads both
        rows.copy_(torch.from_numpy(src))
        d_frames.fill_(n)
        out.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        eager = PV.launch_preview(rows, spec, d_frames)
        assert torch.equal(out, eager), k
        assert not mismatch(out[0], PC.reference_not_blank(src[0], [n], spec, skip=(len(spec.bones) - 1,))), k
    assert not mismatch(PV.launch_preview(torch.from_numpy(joints[None]).to(dev()), spec)[0], want)


def _harness_spec(sk):
    """The harness calls below ask for joints_unit=True, so the body has its real size (bones of 3-36 cm): at 1.6 m across 56 pixels the
    restatement's pictures meet the not-blank condition, which reference_not_blank asserts on the joints each call returned."""
    return PV.PreviewSpec(sk, 40, 56, camera=PV.Camera.orbit(span=1.6, height=40, width=56), radius=1.0)


def test_synthesize_and_synthesize_takes_add_the_preview_of_their_joints():
    model, vae = ted_models()
    sk = SK.ted_expressive()
    spec = _harness_spec(sk)
    U, W, Rd = 2, 2, 2
    g = inputs(U, W, 80)
    audio = torch.from_numpy(synth_audio(U, HOP + N, seed=82)).to(dev())
    kw = dict(labels=g["label"], hop_samples=HOP, z=g["z"], joints=sk, joints_unit=True, smooth=(9, 3), joints_fps=(15, 30))
    plain = Hs.synthesize((model, vae), audio, g["text"], g["seed_pose"], **kw)
    got = Hs.synthesize((model, vae), audio, g["text"], g["seed_pose"], preview=spec, **kw)
    assert set(got) == set(plain) | {"preview"}
    for k, v in plain.items():
        assert torch.equal(got[k], v) if isinstance(v, torch.Tensor) else got[k] == v, k
    T2 = 2 * (W * H_ + P_)
    assert got["joint_frames"] == [T2] * U and tuple(got["preview"].shape) == (U, T2, 40, 56, 3) and got["preview"].dtype == torch.uint8
    assert torch.equal(got["preview"], PV.render_joints(got["joints"], spec, got["joint_frames"]))
    # the pictures are those of the definition: the restatement on the joints the call returned (two frames of each recording)
    pick = got["joints"][:, [0, T2 // 2, T2 - 1]].cpu().numpy()
    assert not mismatch(got["preview"][:, [0, T2 // 2, T2 - 1]], PC.reference_not_blank(pick, None, spec))
    # takes: recordings of unequal length, draws=2, a dict for a spec
    lens = [2 * HOP - 7, HOP - 5]
    audio = torch.from_numpy(synth_audio(U, max(lens), seed=80)).to(dev())
    zz = torch.from_numpy(np.random.default_rng(83).standard_normal((U, Rd, W, 32)).astype(np.float32))
    as_dict = dict(body=sk, height=40, width=56, camera=spec.camera, radius=1.0, layout="chw", colorspace="ycbcr")
    got = Hs.synthesize_takes((model, vae), audio, g["text"], g["seed_pose"], g["label"][:, 0].contiguous(), lengths=lens, draws=Rd, z=zz,
                              hop_samples=HOP, joints=sk, joints_unit=True, smooth=(9, 3), joints_fps=(15, 30), preview=as_dict)
    frames = got["joint_frames"]
    assert got["windows_per"] == [2, 1] and frames == [2 * (w * H_ + P_) for w in (2, 1)]
    assert tuple(got["preview"].shape) == (U, Rd, frames[0], 3, 40, 56)
    assert torch.equal(got["preview"], PV.render_joints(got["joints"], PV.PreviewSpec(**as_dict), frames))
    assert not got["preview"][1, :, frames[1]:].any()
    # the first and the last valid frame of every take against the restatement, whose own pictures must not be blank
    chw = PV.PreviewSpec(**as_dict)
    for u in range(U):
        ends = [0, frames[u] - 1]
        assert not mismatch(got["preview"][u][:, ends], PC.reference_not_blank(got["joints"][u][:, ends].cpu().numpy(), None, chw)), u


def test_the_harness_refusals_fire_before_any_launch():
    model, vae = ted_models()
    sk = SK.ted_expressive()
    spec = _harness_spec(sk)
    U, W = 2, 2
    g = inputs(U, W, 80)
    audio = torch.from_numpy(synth_audio(U, HOP + N, seed=82)).to(dev())
    lib = L.load()
    lens = [2 * HOP - 7, HOP - 5]
    zz = torch.from_numpy(np.random.default_rng(83).standard_normal((U, 2, W, 32)).astype(np.float32))
    calls = ((Hs.synthesize, (g["label"],), dict(z=g["z"])), (Hs.synthesize_takes, (g["label"][:, 0].contiguous(),), dict(lengths=lens, draws=2, z=zz)))
    other = SK.Skeleton(sk.parents.tolist(), sk.children.tolist(), (sk.lengths * 1.5).tolist())
    T2 = 2 * (W * H_ + P_)
    for fn, args, extra in calls:
        rows = U * extra.get("draws", 1)
        too_small = PV.PreviewSpec(sk, 40, 56, max_bytes=rows * T2 * 40 * 56 * 3 - 1)
        for kw, word in ((dict(preview=spec), "preview= without joints="),
                         (dict(preview=PV.PreviewSpec(other, 40, 56), joints=sk), "joints= is Skeleton"),
                         (dict(preview=too_small, joints=sk, joints_fps=(15, 30)), f"{rows} takes x {T2} frames.*max_bytes=.*fewer takes per call")):
            before = int(lib.eg_launch_count())
            with pytest.raises(L.EgError, match=word):
                fn((model, vae), audio, g["text"], g["seed_pose"], *args, hop_samples=HOP, **extra, **kw)
            assert int(lib.eg_launch_count()) == before, (fn.__name__, word)
