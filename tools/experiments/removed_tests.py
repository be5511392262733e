"""Tests of the experiments in this directory as they stood when the kernels were in the product library (rounds 5 to 8).  Not collected by pytest
(not under tests/); they need the kernels pasted or patched back as the README says."""

def test_conv32_teams_kernel_is_bitwise_the_persistent_kernel(monkeypatch):
    """csrc/conv.hip conv3x3_c32_teams_kernel (EG_CONV32_TEAMS = 2 | 3: teams of 4 waves per workgroup sharing ONE LDS copy of the 9 taps' weights,
    3 waves per SIMD) against the default persistent 32 -> 32 kernel: same arithmetic and summation order per output element, so identical bits --
    with the fused SE tail (gate + residual + ReLU in the epilogue), with the pooling partials, and on a tile count that leaves some teams idle."""
    from emotiongestures_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(5)
    for (B, H, W) in ((3, 128, 124), (1, 20, 40), (5, 37, 33)):
        x = torch.randn(B, H, W, 32, generator=g).to(dev)
        w = (torch.randn(32, 32, 3, 3, generator=g) * 0.05)
        res = torch.randn(B, H, W, 32, generator=g).to(dev)
        wp = ops.pack_conv3x3_weight(w, dev)[0]
        outs = {}
        for teams in (None, "2", "3"):
            if teams is None:
                monkeypatch.delenv("EG_CONV32_TEAMS", raising=False)
            else:
                monkeypatch.setenv("EG_CONV32_TEAMS", teams)
            y, gap = ops.conv3x3(x, w, relu=True, want_gap=True, precision="bf16x3", packed=(wp, None, None, None))
            outs[teams] = (y.clone(), gap.clone())
        for teams in ("2", "3"):
            assert torch.equal(outs[teams][0], outs[None][0]) and torch.equal(outs[teams][1], outs[None][1]), (B, H, W, teams)
    # the whole generator (stage 1: six 32 -> 32 convolutions, three of them with the fused SE tail: gate + residual + ReLU in the epilogue)
    from conftest import build_mirror
    from emotiongestures_amd.synth import synth_inputs
    model = build_mirror("spatial", 34, 126, 4, 4, seed=4, precision="bf16x3").to(dev)
    inp = {k: torch.from_numpy(v).to(dev) for k, v in synth_inputs(3, seed=4).items()}
    poses = {}
    for teams in (None, "3"):
        if teams is None:
            monkeypatch.delenv("EG_CONV32_TEAMS", raising=False)
        else:
            monkeypatch.setenv("EG_CONV32_TEAMS", teams)
        with torch.no_grad():
            poses[teams] = model(inp["spec"], inp["text"], inp["pre_pose"], inp["sampled"])[0].clone()
    assert torch.equal(poses["3"], poses[None])



def test_fused_ffn_slab_kernel_matches_the_two_launch_path(monkeypatch):
    """csrc/ffn.hip (opt-in: EG_FFN_FUSED): PositionwiseFeedForward as one slab kernel with the hidden in LDS.  One workgroup per slab ("1") is BITWISE
    the default two pre-split launches (same products per element in the same order, the hidden split by the same function); with the hidden split
    over 4 workgroups per slab ("4") the partial sums are folded by the LayerNorm in a fixed order: equal within 2e-5 at the pose, and repeatable."""
    model = build_mirror("spatial", 34, 126, 4, 4, seed=13, precision="bf16x3").to(dev())
    inp = synth_inputs(8, seed=13)
    g = {k: torch.from_numpy(v).to(dev()) for k, v in inp.items()}

    def run(mode):
        if mode is None:
            monkeypatch.delenv("EG_FFN_FUSED", raising=False)
        else:
            monkeypatch.setenv("EG_FFN_FUSED", mode)
        with torch.no_grad():
            return model(g["spec"], g["text"], g["pre_pose"], g["sampled"])[0].clone()
    ref, one, four, four_again = run(None), run("1"), run("4"), run("4")
    assert torch.equal(one, ref)
    assert torch.equal(four, four_again) and not torch.equal(four, ref)
    assert clip_rel_l2(four.cpu().numpy(), ref.cpu().numpy()) < 2e-5          # another summation order over the hidden chunks, six FFNs deep (measured 8e-6)


# ---- round 10: the convolution's (tile, chunk) walk (conv_tile_walk.patch); from tests/test_gpu_block_entry.py, whose T, dev, _case and _fused they use ----

class _grid:
    """EG_CONV_GRID for the calls inside the block (the library reads it per call): '0' = one workgroup per tile, N = N persistent workgroups."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        import os
        self.old = os.environ.pop("EG_CONV_GRID", None)
        if self.value is not None:
            os.environ["EG_CONV_GRID"] = str(self.value)

    def __exit__(self, *exc):
        import os
        os.environ.pop("EG_CONV_GRID", None)
        if self.old is not None:
            os.environ["EG_CONV_GRID"] = self.old


# 64 -> 64 at 20 x 37: 3 x 2 tiles per clip, 18 in all: 8 workgroups walk 3 or 2 tiles each, 24 leave six without a tile; the stride-2 entries at
# 37 x 69 -> 19 x 35: 10 x 2 tiles per clip (2-row tiles); final_conv1 128 -> 34 with the NCHW epilogue at 20 x 31: 5 tiles per clip
PERSIST_CASES = [(64, 64, 1, 20, 37, False), (32, 64, 2, 37, 69, False), (64, 128, 2, 37, 69, False), (128, 34, 1, 20, 31, True)]


@pytest.mark.parametrize("prec", ["bf16x3", "bf16"])
@pytest.mark.parametrize("cin,cout,stride,H,W,nchw", PERSIST_CASES)
def test_persistent_walk_is_bitwise_the_tile_per_workgroup_launch(cin, cout, stride, H, W, nchw, prec):
    from emotiongestures_amd import ops
    B = 3
    x = T(f"px{cin}", (B, H, W, cin), -1, 1).to(dev())
    w = T(f"pw{cin}{cout}", (cout, cin, 3, 3), -0.1, 0.1)
    bias, scale, shift = T("b", (cout,), -0.2, 0.2), T("s", (cout,), 0.5, 1.5), T("t", (cout,), -0.3, 0.3)
    packed = ops.conv3x3_pack(w, bias, scale, shift, dev())

    def run(grid):
        with _grid(grid):
            y, gap = ops.conv3x3(x, w, stride=stride, relu=True, nchw_out=nchw, want_gap=True, precision=prec, packed=packed)
        torch.cuda.synchronize()
        return y, gap

    y0, g0 = run(0)
    assert torch.isfinite(y0).all() and float(y0.abs().max()) > 0
    for grid in (8, 24, None):
        y, g = run(grid)
        assert torch.equal(y, y0), grid
        assert torch.equal(g, g0), grid


@pytest.mark.parametrize("prec", ["bf16x3", "bf16"])
def test_persistent_walk_carries_the_shortcut_pre_phase(prec):
    """layer2.0 in the fused flow (conv2 = the 64 -> 64 kernel with the shortcut steps first in every tile's sequence): 3 clips, 19 x 35 output."""
    blk, x, _ref = _case("layer2", 37, 69, True)
    outs = []
    for grid in (0, 8, 24, None):
        with _grid(grid):
            outs.append(_fused(blk, x, prec))
    for o in outs[1:]:
        assert torch.equal(o, outs[0])


# ---- round 10: the 128 x 128 tile with 64-deep steps (gemm_presplit_tiles.patch); from tests/test_gpu_causal_product.py, whose T, dev and
# split_images it uses.  The same patch brings back the "64r8", "128x64", "128x64r3", "128x64r6" and "128r4" entries of the tile list of
# tests/test_gpu_kernels.py::test_linear_presplit_tile_variants_are_bitwise_equal ----

@pytest.mark.parametrize("prec", ["bf16x3", "bf16"])
@pytest.mark.parametrize("M,N,K", [(136, 512, 512), (2176, 128, 2048), (200, 192, 96)])
def test_presplit128_64_deep_steps_bitwise_equal(prec, M, N, K, monkeypatch):
    """EG_GEMM_TILE=128k64 (128 x 128 tile, 64-deep steps, two-slot ring) keeps the K order of every output element: bitwise the 32-deep
    128 x 128 kernel, with bias + residual + ReLU; K = 96 ends on an odd 32 (half a last step), 200 x 192 has odd tile counts on both axes."""
    from emotiongestures_amd import _lib as L
    from emotiongestures_amd import ops
    from emotiongestures_amd.engine import _ptr, _stream
    lib = L.load()
    x, w = T("kx", (M, K)), T("kw", (N, K), -0.1, 0.1)
    bias, res = T("kb", (N,)), T("kr", (M, N))
    xd, rd = x.to(dev()), res.to(dev())
    wp, npad, kpad = ops.pack_linear_weight(w, dev())
    bp = torch.zeros(npad, device=dev())
    bp[:N] = bias.to(dev())
    img = split_images(xd, M, K)
    outs = {}
    for tile in ("128", "128k64"):
        monkeypatch.setenv("EG_GEMM_TILE", tile)
        y = torch.full((M, N), float("nan"), device=dev())
        L.check(lib.eg_linear_presplit(_ptr(img), K, _ptr(wp), kpad, _ptr(bp), _ptr(rd), None, N, _ptr(y), N, M, N, K, 1,
                                       L.precision_code(prec), _stream(dev())), "eg_linear_presplit " + tile)
        torch.cuda.synchronize()
        outs[tile] = y
    monkeypatch.delenv("EG_GEMM_TILE")
    ref = torch.relu(x.double() @ w.double().T + bias.double() + res.double())
    assert rel_l2(outs["128"].cpu().numpy(), ref.numpy()) < {"bf16x3": 3e-5, "bf16": 2e-2}[prec]
    assert torch.equal(outs["128k64"], outs["128"])


# ---- round 15: the training image chain (activations and gradients handed from product to product as pre-split bf16 (hi, lo) images:
# functional.PRESPLIT_ROWS / presplit_ok / new_images / raw_linear(x_img=, want_img=) / _ln_backward_ex(want_img=), EgLinearArgs::x_images / y_images /
# k_x / y_k, eg_layernorm_backward_ex's branch_images).  From tests/test_gpu_training.py, whose T, DEV and rel they use; they need the files of the
# parent commit named in README.md ----

def linear_ex_presplit_tail(F, L, _ptr, _stream, precision, M, K, N, x, w, b, gate, site, res, both):
    """The end of the shape loop of test_linear_ex_epilogue_masks_match_the_separate_kernels: the pre-split product with the training epilogue
    (gemm_presplit_kernel<3, true>, gemm_presplit128_kernel<3, true>, gemm_skinny_kernel<1..4, false, true>) against the fp32-input kernel."""
    if precision == "bf16x3" and K % 64 == 0 and N % 64 == 0:
        # the pre-split product (X through images, both operands by LDS-DMA) with the same epilogue, and Y leaving as images for the next one
        ximg = F.new_images(M, K, DEV)
        L.check(L.load().eg_split_tiles(_ptr(x), K, M, K, _ptr(ximg), _stream(DEV)), "eg_split_tiles")
        got_p, yimg = F.raw_linear(x, w, b, gate=gate, drop=site, res=res, relu=True, x_img=ximg, want_img=True)
        # bitwise the fp32-input kernel's result unless that one took its split-K path (another summation order over K)
        assert torch.equal(got_p, both) if K < 1024 else rel(got_p, both) < 1e-6
        want_y = torch.zeros_like(yimg)
        L.check(L.load().eg_split_tiles(_ptr(got_p), N, M, N, _ptr(want_y), _stream(DEV)), "eg_split_tiles")
        mt = (M + 63) // 64
        a16, b16 = yimg.view(torch.int16).view(2, mt, N // 8, 64, 8), want_y.view(torch.int16).view(2, mt, N // 8, 64, 8)
        for t in range(mt):
            r = min(64, M - t * 64)
            assert torch.equal(a16[:, t, :, :r], b16[:, t, :, :r])


def layernorm_backward_ex_image_tail(F, L, _ptr, _stream, x, dy, gp, bp, site, dbr, rows, D):
    """The end of test_layernorm_backward_ex_matches_torch_and_the_dropout_kernel: ln_bwd_ex_kernel's image store against eg_split_tiles of dbr."""
    # the branch gradient as pre-split images (for the input-gradient product that follows in large-batch steps): the split eg_split_tiles makes of it
    with F.precision("bf16x3"):
        old, F.PRESPLIT_ROWS = F.PRESPLIT_ROWS, 1
        try:
            img = F._ln_backward_ex(x.to(DEV), dy.to(DEV), gp.detach(), 1e-6, site, gp, bp, want_img=True)[4]
        finally:
            F.PRESPLIT_ROWS = old
    want_img = torch.zeros_like(img)
    L.check(L.load().eg_split_tiles(_ptr(dbr), D, rows, D, _ptr(want_img), _stream(DEV)), "eg_split_tiles")
    mt, n_valid = (rows + 63) // 64, None
    a16, b16 = img.view(torch.int16).view(2, mt, D // 8, 64, 8), want_img.view(torch.int16).view(2, mt, D // 8, 64, 8)
    for t in range(mt):                 # rows past the end of the last tile are not written by the LayerNorm kernel (never read as results)
        r = min(64, rows - t * 64)
        assert torch.equal(a16[:, t, :, :r], b16[:, t, :, :r])


# test_fused_blocks_step_equals_the_operator_by_operator_step had a fifth parameter `chain` and the row ("bf16x3", True, True, True); inside run(seed):
#         F.PRESPLIT_ROWS = 64 if chain else 1 << 30        (before the `try`)
#             F.PRESPLIT_ROWS = old_rows                     (in the `finally`, old_rows read before run was defined)
# i.e. the large-batch mode forced at 102 rows: activations handed from block to block as images, checked like the four rows that remain.
