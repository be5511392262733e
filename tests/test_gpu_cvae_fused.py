"""eg_cvae_sample in one launch (csrc/misc.hip: cvae_sample_fused_kernel) against the launch chain it replaces (EG_CVAE_FUSED=0), bit for bit:
the fused kernel keeps every output element's summation order, the MLP head's included, so torch.equal is the check.  The shapes are the
places where a tiled halo walk goes wrong: several tiles, a partial last tile, an axis of one short tile, and out-of-range halo positions
that must be the next stage's zero padding."""
import pytest
import torch

from emotiongestures_amd import _lib
from emotiongestures_amd.CAVE.BEAT_CVAE import MLP_Reconstruct_v3
from emotiongestures_amd.synth import load_synth_weights, synth_inputs

pytestmark = pytest.mark.gpu
CHAIN_LAUNCHES = 10         # 2 + 2 small linears, the z copy, 2 transposed and 3 plain convolutions


def dev():
    return torch.device("cuda:0")


def model(F, D, seed, big_bias=False):
    m = load_synth_weights(MLP_Reconstruct_v3(frames=F, d_model=D), seed).eval()
    if big_bias:        # every bias and every BatchNorm shift large: a halo position computed from the bias instead of stored as 0 shows
        with torch.no_grad():
            for k, v in m.state_dict().items():
                if k.endswith(".bias"):
                    v.fill_(1e3)
    return m.to(dev())


def inputs(n, F, D, seed):
    inp = synth_inputs(n, F, d_model=D, seed=seed)
    return torch.from_numpy(inp["label"]).to(dev()), torch.from_numpy(inp["z"]).to(dev())


def both_paths(m, y, z, monkeypatch, fused_launches=1):
    """sample() on the default path and on the launch chain; the library's launch counter says which path each call took."""
    lib = _lib.load()
    with torch.no_grad():
        monkeypatch.delenv("EG_CVAE_FUSED", raising=False)
        c0 = lib.eg_launch_count()
        fused = m.sample(y, z=z).clone()
        c1 = lib.eg_launch_count()
        monkeypatch.setenv("EG_CVAE_FUSED", "0")
        chain = m.sample(y, z=z).clone()
        c2 = lib.eg_launch_count()
        monkeypatch.delenv("EG_CVAE_FUSED")
    torch.cuda.synchronize()
    assert (c1 - c0, c2 - c1) == (fused_launches, CHAIN_LAUNCHES)
    return fused, chain


@pytest.mark.parametrize("n,F,D", [(3, 34, 512), (2, 60, 512), (1, 60, 192), (5, 34, 64), (2, 120, 512)])
def test_fused_sample_is_the_chain_bit_for_bit(n, F, D, monkeypatch):
    """(3,34,512) several tiles and an odd batch; (1,60,192) a partial last tile; (5,34,64) the axis is one short tile and z0 is 16 positions
    long; (2,120,512) does NOT run fused (the last stage's weights exceed the LDS): it checks that the silent fall-back is the chain."""
    m = model(F, D, 11)
    y, z = inputs(n, F, D, 11)
    fused, chain = both_paths(m, y, z, monkeypatch, fused_launches=CHAIN_LAUNCHES if F == 120 else 1)
    assert tuple(fused.shape) == (n, F, D) and bool(torch.isfinite(chain).all())
    diff = (fused - chain).abs().max().item()
    assert torch.equal(fused, chain), f"fused differs from the chain: max |d| {diff:.3e} at scale {chain.abs().max().item():.3e}"


def test_halo_positions_outside_the_axis_are_zero_padding(monkeypatch):
    m = model(34, 192, 5, big_bias=True)
    y, z = inputs(1, 34, 192, 5)
    fused, chain = both_paths(m, y, z, monkeypatch)
    assert bool(torch.isfinite(chain).all())
    bad = (fused != chain).nonzero()
    assert torch.equal(fused, chain), f"{bad.shape[0]} elements differ, first at (n, f, l) = {bad[0].tolist() if bad.shape[0] else None}"


def test_two_lanes_replayed_from_graphs_equal_the_eager_calls(monkeypatch):
    """Two sample() calls with their own slot, stream and inputs, each captured as bench.py's diversity leg captures a lane, replayed
    alternately: the fused path keeps no state that the lanes could share."""
    from emotiongestures_amd.pipeline import CAPTURE_MODE
    monkeypatch.delenv("EG_CVAE_FUSED", raising=False)
    m = model(34, 512, 2)
    ins = [inputs(4, 34, 512, 20 + i) for i in range(2)]
    with torch.no_grad():
        eager = [m.sample(y, z=z).clone() for y, z in ins]
    assert not torch.equal(eager[0], eager[1])
    graphs = []
    for i, (y, z) in enumerate(ins):
        st = torch.cuda.Stream(dev())
        st.wait_stream(torch.cuda.current_stream(dev()))
        with torch.cuda.stream(st), torch.no_grad():
            m.sample(y, z=z, slot=i)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=st, capture_error_mode=CAPTURE_MODE), torch.no_grad():
            out = m.sample(y, z=z, slot=i)
        graphs.append((gr, st, out))
    for _ in range(3):
        for gr, st, out in graphs:
            out.fill_(float("nan"))
        torch.cuda.synchronize()
        for gr, st, out in graphs:
            with torch.cuda.stream(st):
                gr.replay()
        torch.cuda.synchronize()
        for (gr, st, out), want in zip(graphs, eager):
            assert torch.equal(out, want)
