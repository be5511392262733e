"""BVH text of whole takes on the GPU (csrc/bvhtext.hip through emotiongestures_amd.bvh.format_tracks / TextKernels and
harness.synthesize(bvh_text=True)): the bytes against the integer restatement tests/bvh_text_np.py and against ``BvhFile.format`` per take.
Everything is exact: bytes are equal or they are not.  The only tolerance is the round trip's 5e-7, half a unit of the sixth decimal."""
import numpy as np
import pytest
import torch

import articulate_np as AN
import bvh_text_np as TN
from emotiongestures_amd import _lib as L
from emotiongestures_amd import bvh as BVH
from emotiongestures_amd import harness as Hs

pytestmark = pytest.mark.gpu

TF = BVH.TEXT_TILE_FRAMES
TWO_POSITIONS = "Yposition Xposition Zrotation Xrotation Yrotation"
WIDTH_VALUE = {8: 1.0, **{w: -(10.0 ** (w - 9)) for w in range(9, 19)}}                 # a value whose text has w bytes
GUARD = 64


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def small(root_channels=None):
    text = TN.SMALL
    if root_channels is not None:
        text = text.replace("CHANNELS 6 Xposition Yposition Zposition Zrotation Xrotation Yrotation",
                            f"CHANNELS {len(root_channels.split())} {root_channels}")
    return BVH.parse(text)


def tracks(rows, T, J3, seed, scale=150.0):
    """fp32 [rows, T, J3] and root positions [rows, T, 3]: random angles, and in the first and the last frame of every tile the special
    values, walking through the channel positions."""
    rng = np.random.default_rng(seed)
    sp = TN.special_values()
    e = (rng.standard_normal((rows, T, J3)) * scale).astype(np.float32)
    rp = (rng.standard_normal((rows, T, 3)) * 40).astype(np.float32)
    for b in range(rows):
        for t in range(T):
            if t % TF in (0, TF - 1):
                e[b, t] = sp[(np.arange(J3) + t + 5 * b) % len(sp)]
                rp[b, t] = sp[(np.arange(3) + 7 * t + b) % len(sp)]
    return e, rp


def run_kernels(f, e, frames, draws, rp, joints=None):
    """measure, sizes, write into a guarded buffer -> (bytes, offsets, line_off) with the guard checked."""
    x = gpu(e)
    fr = None if frames is None else list(frames)
    d_frames = None if fr is None else torch.tensor(fr, dtype=torch.int32, device=dev())
    k = BVH.TextKernels(f.text_table(joints, rp is not None), x, fr, d_frames, draws, None if rp is None else gpu(rp))
    k.measure()
    total, offsets = k.sizes()
    text = torch.full((total + GUARD,), 0xAA, dtype=torch.uint8, device=dev())
    k.write(text)
    host = text.cpu().numpy()
    assert (host[total:] == 0xAA).all(), "bytes behind the last take were written"
    return host[:total].tobytes(), offsets, k.line_off.cpu().numpy()


def test_one_take_equals_format():
    f = small()
    e, rp = tracks(1, 3, 12, 1)
    x = gpu(e[0].reshape(3, 4, 3))
    bt = f.format_tracks(x, frame_time=1 / 30, root_position=gpu(rp[0]))
    assert bt.lead == () and bt.body.is_cuda and bt.body.dtype == torch.uint8 and bt.frames == [3] and list(bt.offsets) == [0, bt.body.numel()]
    assert bt.text() == f.format(e[0].reshape(3, 4, 3), frame_time=1 / 30, root_position=rp[0])
    assert bt.text().count("\n") == TN.SMALL.count("\n") + 3 + 3 and "-0.000000" in bt.text()


@pytest.mark.parametrize("T", [TF - 1, TF, TF + 1, 2 * TF + 3])
def test_batch_bytes_offsets_and_every_alignment(T):
    """[2, 2, T, J, 3] with frames [T, 5] and NaN behind the valid frames.  The first line of the first row grows by 0 .. 15 bytes over sixteen
    runs, so the start of every later row and tile takes every residue modulo 16: the head and tail byte stores and the 16-byte interior
    of the write kernel at every alignment."""
    f = small()
    U, R = 2, 2
    frames = [T, 5]
    per_row = [T, T, 5, 5]
    e, rp = tracks(U * R, T, 12, 20 + T)
    rp = rp[::R].copy()
    e[2:, 5:] = np.nan
    rp[1, 5:] = np.nan
    src = f._channel_sources(f._rotating(None, "test"), True)
    row_res, tile_res = set(), set()
    for shift in range(16):
        w0 = 8 + min(shift, 10)
        e[0, 0, 0], e[0, 0, 1] = WIDTH_VALUE[w0], WIDTH_VALUE[16 + shift - w0]
        want, want_off, want_lines = TN.body(src, e, per_row, rp, R)
        got, off, lines = run_kernels(f, e, frames, R, rp)
        assert np.array_equal(off, want_off) and np.array_equal(lines, want_lines)
        assert got == want
        row_res |= {int(o) % 16 for o in off[1:-1]}
        tile_res |= {int(lines[b * T + t]) % 16 for b in range(U * R) for t in range(0, per_row[b], TF) if b or t}
        if shift in (0, 9):
            bt = f.format_tracks(gpu(e.reshape(U, R, T, 4, 3)), frames, frame_time=0.02, root_position=gpu(rp))
            assert np.array_equal(bt.offsets, want_off) and bt.host().tobytes() == want
            for u in range(U):
                for r in range(R):
                    assert bt.text(u, r) == f.format(e[u * R + r, :frames[u]].reshape(-1, 4, 3), frame_time=0.02, root_position=rp[u, :frames[u]])
    assert row_res == set(range(16)) and tile_res == set(range(16))


@pytest.mark.parametrize("root_channels", [None, TWO_POSITIONS])
def test_joints_subset_and_root_position_given_or_absent(root_channels):
    f = small(root_channels)
    T = TF + 2
    for joints in (None, ["Hips", "Leg"], ["Arm"]):
        J = 4 if joints is None else len(joints)
        e, rp = tracks(3, T, 3 * J, 40 + J)
        for root in (None, rp):
            bt = f.format_tracks(gpu(e.reshape(3, T, J, 3)), [T, 1, TF], joints=joints, frame_time=1 / 15, root_position=None if root is None else gpu(root))
            for u, n in enumerate([T, 1, TF]):
                want = f.format(e[u, :n].reshape(n, J, 3), joints, 1 / 15, None if root is None else root[u, :n])
                assert bt.text(u) == want, (joints, root is None, u)


def wide_file():
    """512 channels: a root with two position channels and 169 joints of three."""
    joints = "".join(f"  JOINT j{i}\n  {{\n    OFFSET {i}.5 0.0 -{i}.25\n    CHANNELS 3 Zrotation Xrotation Yrotation\n  }}\n" for i in range(169))
    f = BVH.parse(f"HIERARCHY\nROOT r\n{{\n  OFFSET 0 0 0\n  CHANNELS 5 {TWO_POSITIONS}\n{joints}}}\n")
    assert f.channels == TN.MAX_CHANNELS
    return f


def test_widest_file_fills_the_tile_of_lds():
    """C = 512 at T = tile + 1, every value 18 bytes wide: a full tile is TF * 512 * 19 bytes, the bound the LDS of a workgroup is sized for;
    one short value ahead of row 1 moves its tiles off the 16-byte grid, which is what the 16 spare bytes are for."""
    f = wide_file()
    T = TF + 1
    e = np.full((2, T, 510), WIDTH_VALUE[18], np.float32)
    e -= np.arange(510, dtype=np.float32)[None, None] * 128                          # distinct values of the same width
    rp = np.full((2, T, 3), -2147483520.0, np.float32)
    e[0, T - 1, 7] = 1.0
    got, off, lines = run_kernels(f, e, None, 1, rp)
    assert lines[TF] - lines[0] == TF * 512 * 19 and int(off[1]) % 16 != 0 and lines[T + TF] - lines[T] == TF * 512 * 19
    for b in range(2):
        want = f.format(e[b].reshape(T, 170, 3), frame_time=1.0, root_position=rp[b])
        assert want.encode().endswith(got[off[b]:off[b + 1]]) and got[off[b]:off[b + 1]].count(b"\n") == T


def test_a_row_does_not_depend_on_its_batch():
    f = small()
    T = 2 * TF + 3
    e, rp = tracks(4, T, 12, 60)
    rp = rp[::2].copy()
    whole = f.format_tracks(gpu(e.reshape(2, 2, T, 4, 3)), [T, TF + 2], frame_time=0.1, root_position=gpu(rp))
    n = TF + 2
    alone = f.format_tracks(gpu(e[2, :n].reshape(n, 4, 3)), frame_time=0.1, root_position=gpu(rp[1, :n]))        # another T, another place
    assert alone.text() == whole.text(1, 0)
    assert alone.host().tobytes() == whole.host()[whole.offsets[2]:whole.offsets[3]].tobytes()


def test_values_that_are_not_writable_are_refused_by_name():
    f = small()
    T = TF + 1
    e, rp = tracks(4, T, 12, 70)
    x = e.reshape(2, 2, T, 4, 3).copy()
    x[1, 0, 2, 1, 0] = np.nan
    x[1, 0, T - 1, 3, 2] = np.inf
    x[1, 1, 0, 0, 0] = np.nan
    with pytest.raises(L.EgError, match=r"BvhFile.format_tracks: take \[1, 0\] \(row 2\) has 2 values in its valid frames that are NaN, infinite or >= 2\^31"):
        f.format_tracks(gpu(x), frame_time=0.1)
    x = e.reshape(2, 2, T, 4, 3).copy()
    x[0, 1, TF, 2, 1] = 2.0 ** 31
    with pytest.raises(L.EgError, match=r"take \[0, 1\] \(row 1\) has 1 values"):
        f.format_tracks(gpu(x), frame_time=0.1)
    x[0, 1, TF, 2, 1] = -(2.0 ** 31)
    with pytest.raises(L.EgError, match=r"row 1 has 1 values"):
        f.format_tracks(gpu(x.reshape(4, T, 4, 3)), frame_time=0.1)
    bad_root = rp[::2].copy()
    bad_root[1, 3, 2] = -np.inf
    with pytest.raises(L.EgError, match=r"take \[1, 0\] \(row 2\) has 1 values"):
        f.format_tracks(gpu(e.reshape(2, 2, T, 4, 3)), frame_time=0.1, root_position=gpu(bad_root))
    x = e.reshape(2, 2, T, 4, 3).copy()                                            # behind the valid frames nothing is counted
    x[1, :, 3:] = np.nan
    assert f.format_tracks(gpu(x), [T, 3], frame_time=0.1).text(1, 1) == f.format(x[1, 1, :3], frame_time=0.1)


def test_graph_replay_equals_the_eager_calls():
    f = small()
    rows, T = 3, 2 * TF + 3
    fr = [T, TF + 1, 2]
    e0, rp0 = tracks(rows, T, 12, 80)
    e1, rp1 = tracks(rows, T, 12, 81, scale=3000.0)
    x, root = gpu(e0), gpu(rp0)
    d_frames = torch.tensor(fr, dtype=torch.int32, device=dev())
    k = BVH.TextKernels(f.text_table(None, True), x, fr, d_frames, 1, root)
    text = torch.zeros(rows * T * 18 * 19, dtype=torch.uint8, device=dev())
    k.measure()
    k.write(text)                                                                  # warm-up
    torch.cuda.synchronize()
    graphs = []
    for fn in (k.measure, lambda: k.write(text)):                                  # one graph each: the caller reads the sizes in between
        g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s), torch.cuda.graph(g, stream=s):
            fn()
        torch.cuda.current_stream().wait_stream(s)
        graphs.append(g)
    x.copy_(gpu(e1)); root.copy_(gpu(rp1)); text.zero_()
    graphs[0].replay()
    total, offsets = k.sizes()
    graphs[1].replay()
    torch.cuda.synchronize()
    eager = f.format_tracks(gpu(e1.reshape(rows, T, 4, 3)), fr, frame_time=0.1, root_position=gpu(rp1))
    assert total == eager.body.numel() and np.array_equal(offsets, eager.offsets)
    assert torch.equal(text[:total], eager.body) and not text[total:].any()


def test_round_trip_through_the_parser():
    f = small()
    T = TF + 3
    rng = np.random.default_rng(90)
    e = (rng.uniform(-180, 180, (2, T, 4, 3))).astype(np.float32)
    rp = (rng.standard_normal((2, T, 3)) * 100).astype(np.float32)
    bt = f.format_tracks(gpu(e), [T, TF], frame_time=1 / 60, root_position=gpu(rp))
    for u, n in enumerate([T, TF]):
        back = BVH.parse(bt.text(u))
        assert back.frames == n and back.frame_time == pytest.approx(1 / 60, abs=5e-7)
        assert np.abs(back.euler() - e[u, :n].astype(np.float64)).max() <= 5e-7
        assert np.abs(back.root_position() - rp[u, :n].astype(np.float64)).max() <= 5e-7


def test_c_abi_clamps_values_that_are_not_writable():
    """Called anyway through the kernels' own wrapper, NaN and 2^31 are written as 0.000000 and counted."""
    f = small()
    e, _rp = tracks(1, 2, 12, 95)
    e[0, 1, 4], e[0, 0, 11] = np.nan, 2.0 ** 31
    x = gpu(e)
    k = BVH.TextKernels(f.text_table(), x)
    k.measure()
    with pytest.raises(L.EgError, match="row 0 has 2 values"):
        k.sizes()
    total = int(k.summary[0].item())
    text = torch.zeros(total, dtype=torch.uint8, device=dev())
    k.write(text)
    e[0, 1, 4] = e[0, 0, 11] = 0.0
    assert text.cpu().numpy().tobytes().decode() == f.format(e[0].reshape(2, 4, 3), frame_time=1.0).split("Frame Time: 1.000000\n")[1]


# ---- the harness -----------------------------------------------------------------------------------------------------------------------------
def upper47_bvh():
    parents = AN.BODIES["upper47"]()[0]
    kids = {j: [k for k, p in enumerate(parents) if p == j] for j in range(len(parents))}

    def node(j, pad):
        head = "ROOT" if j == 0 else "JOINT"
        ch = "CHANNELS 6 Xposition Yposition Zposition Zrotation Xrotation Yrotation" if j == 0 else "CHANNELS 3 Zrotation Xrotation Yrotation"
        inner = "".join(node(k, pad + "  ") for k in kids[j]) or f"{pad}  End Site\n{pad}  {{\n{pad}    OFFSET 0.0 2.0 0.0\n{pad}  }}\n"
        return f"{pad}{head} j{j}\n{pad}{{\n{pad}  OFFSET {0.5 * (j % 5)} {3.0 + j} {-0.25 * (j % 3)}\n{pad}  {ch}\n{inner}{pad}}}\n"
    return BVH.parse("HIERARCHY\n" + node(0, ""))


def test_synthesize_with_bvh_text_equals_format_of_its_euler_channels():
    import test_gpu_euler as TE
    model, vae = TE.beat_models()
    f = upper47_bvh()
    tree = f.tree()
    assert tree.J == 47 and f.channels == 3 * 47 + 3
    U, W = 2, 3
    g = TE.beat_inputs(U, W, 120)
    lengths = [3 * TE.HOP - 100, TE.HOP + 700]
    audio = TE.gpu(TE.synth_audio(U, max(lengths), seed=80))
    zz = torch.from_numpy(TE.hash_uniform("articulate/z", (U, 2, W, 32), -2.0, 2.0, 121))
    kw = dict(hop_samples=TE.HOP, joints=tree, euler=f, labels=g["label"][:, 0].contiguous(), z=zz, draws=2, lengths=lengths, euler_unwrap=True,
              joints_fps=(15, 30))
    out = Hs.synthesize_takes((model, vae), audio, g["text"], g["seed_pose"], bvh_text=True, **kw)
    bt = out["bvh"]
    assert isinstance(bt, BVH.BvhText) and bt.lead == (U, 2) and bt.frames == out["joint_frames"] and bt.body.is_cuda
    eul = out["euler"].cpu().numpy()
    for u in range(U):
        for r in range(2):
            n = out["joint_frames"][u]
            assert bt.text(u, r) == f.format(eul[u, r, :n], joints=tree.names, frame_time=1 / 30)
    plain = Hs.synthesize_takes((model, vae), audio, g["text"], g["seed_pose"], **kw)
    assert set(out) == set(plain) | {"bvh"} and torch.equal(plain["euler"], out["euler"])
    one = Hs.synthesize((model, vae), audio[:, :2 * TE.HOP + TE.NS].contiguous(), g["text"], g["seed_pose"], hop_samples=TE.HOP, joints=tree, euler=f,
                        labels=g["label"], z=g["z"], bvh_text=True)
    assert one["bvh"].lead == (U,) and one["bvh"].text(1) == f.format(one["euler"][1].cpu().numpy(), joints=tree.names, frame_time=1 / 15)
    for fn, extra in ((Hs.synthesize, dict(labels=g["label"], z=g["z"])), (Hs.synthesize_takes, dict(labels=g["label"][:, 0].contiguous(), z=zz, draws=2))):
        with pytest.raises(L.EgError, match=f"{fn.__name__}: bvh_text=True needs euler=BvhFile"):
            fn((model, vae), audio, g["text"], g["seed_pose"], hop_samples=TE.HOP, joints=tree, euler="ZXY", bvh_text=True, **extra)
        with pytest.raises(L.EgError, match=f"{fn.__name__}: bvh_text=True needs euler=BvhFile"):
            fn((model, vae), audio, g["text"], g["seed_pose"], hop_samples=TE.HOP, bvh_text=True, **extra)
