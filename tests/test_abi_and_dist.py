"""CPU-only checks: the C-ABI library loads and exports every symbol include/emogest.h declares, its weight manifest is
consistent with the reference state_dict schema, host logic (sharding) incl. a world_size-2 gloo run."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, build_mirror


def _header_symbols():
    text = open(os.path.join(ROOT, "include", "emogest.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(eg_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_header_symbol():
    from emotiongestures_amd import _lib
    lib = _lib.load()
    syms = _header_symbols()
    assert len(syms) > 40
    missing = [s for s in syms if not hasattr(lib, s)]
    assert not missing, missing
    unbound = [s for s in syms if s not in _lib.SIGNATURES]
    assert not unbound, f"declared in the header but not bound in _lib.SIGNATURES: {unbound}"
    assert lib.eg_version().startswith(b"emogest-hip")


def test_linear_args_struct_matches_the_header():
    """_lib.EgLinearArgs against `typedef struct EgLinearArgs` of include/emogest.h: the same field names in declaration order, the same width per
    field, and ctypes' size equal to the size the header's list gives when every field sits at its natural alignment."""
    from emotiongestures_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "emogest.h")).read(), flags=re.S)
    body = re.search(r"typedef\s+struct\s+EgLinearArgs\s*\{(.*?)\}\s*EgLinearArgs\s*;", text, flags=re.S).group(1)
    widths = {"uint64_t": 8, "int32_t": 4, "uint32_t": 4, "float": 4}
    header = []                                                     # (name, bytes, kind) in declaration order
    for decl in (d.strip() for d in body.split(";")):
        if not decl:
            continue
        m = re.fullmatch(r"(?:const\s+)?(\w+)\s*(\*?)\s*(.+)", decl, flags=re.S)
        base, star, names = m.group(1), m.group(2), m.group(3)
        for name in (n.strip() for n in names.split(",")):
            if star or name.startswith("*"):
                header.append((name.lstrip("* "), C.sizeof(C.c_void_p), "pointer"))
            else:
                header.append((name, widths[base], base))
    assert len(header) > 20
    kinds = {C.c_void_p: "pointer", C.c_uint64: "uint64_t", C.c_int32: "int32_t", C.c_uint32: "uint32_t", C.c_float: "float"}
    bound = [(n, C.sizeof(t), kinds[t]) for n, t in _lib.EgLinearArgs._fields_]
    assert bound == header
    size = align = 0
    for _n, w, _k in header:
        size = (size + w - 1) // w * w + w
        align = max(align, w)
    assert C.sizeof(_lib.EgLinearArgs) == (size + align - 1) // align * align


def test_manifest_covers_the_state_dict_and_packs_to_declared_sizes():
    """Every parameter that influences the eval forward appears in the manifest; packing fills exactly numel floats."""
    from emotiongestures_amd import packing
    from emotiongestures_amd.engine import GeneratorEngine
    for variant in ("spatial", "memory"):
        m = build_mirror(variant, 34, 126, 4, 4)
        eng = GeneratorEngine(variant=variant)
        sd = m.state_dict()
        used = set()
        for e in eng.entries:
            key = e.key.decode()
            if e.kind in (4, 5):
                used |= {key + s for s in (".weight", ".bias", ".running_mean", ".running_var")}
            elif e.kind == 8:
                used |= {key + ".weight_g", key + ".weight_v"}
            else:
                used |= set(key.split("|"))         # '|' joins tensors packed into one fused image
            assert e.offset % 16 == 0
        assert used <= set(sd), sorted(used - set(sd))[:5]
        # parameters the reference itself never uses in forward (SURVEY §7 hard part 5) are the only ones left out
        unused = [k for k in sd if k not in used and "num_batches_tracked" not in k]
        for k in unused:
            assert any(s in k for s in ("slf_attn", "position_embeddings", "pos_table2", "decoder.position_enc", ".layer_norm.",
                                        "spatial_memory.spatial_chunk_encoder", "net.0.", "net.4.")) or variant == "memory", k
        arena = packing.build_arena(sd, eng.entries, eng.arena_floats)
        assert arena.numel() == eng.arena_floats and torch.isfinite(arena[:1000]).all()


def test_config_validation_and_status_codes():
    from emotiongestures_amd import _lib
    from emotiongestures_amd.engine import GeneratorEngine
    with pytest.raises(_lib.EgError):
        GeneratorEngine(frames=4, prior_frames=4)            # frames must exceed prior_frames
    with pytest.raises(_lib.EgError):
        GeneratorEngine(d_model=500)                         # d_model must be heads*64
    with pytest.raises(ValueError):
        GeneratorEngine(precision="fp8")
    lib = _lib.load()
    assert lib.eg_set_default_precision(7) != 0 and b"precision" in lib.eg_last_error()
    assert lib.eg_conv3x3(None, None, None, None, None, None, None, 1, 8, 8, 32, 32, 1, 0, 0, 0, None) == -1   # EG_ERR_BAD_ARG, no launch
    # argument validation happens before any HIP call, so these run without a GPU: every entry refuses null operands / bad
    # shapes with a negative status and a message, and launches nothing
    one = C.c_void_p(16)                                      # a non-null, 16-byte aligned dummy address that is never dereferenced
    assert lib.eg_linear(None, 4, None, 4, None, None, None, 0, None, 4, 1, 1, 4, 0, 0, 0, 0, None) < 0
    assert lib.eg_layernorm(None, None, None, None, 4, 512, 1e-6, None) < 0
    assert lib.eg_attention(one, 512, one, 512, one, 512, one, 512, None, 1, 8, 4, 4, 32, 0, None) == -2         # d_k 32: EG_ERR_UNSUPPORTED
    assert b"d_k" in lib.eg_last_error()
    assert lib.eg_attention(one, 512, one, 512, one, 512, one, 512, None, 1, 8, 4, 300, 64, 0, None) == -2        # Lk > 256
    assert lib.eg_conv3x3(one, one, None, None, None, one, None, 1, 8, 8, 32, 32, 3, 0, 0, 0, None) == -2      # stride 3
    assert lib.eg_conv3x3(one, one, None, None, None, one, None, 1, 8, 8, 48, 48, 1, 0, 0, 0, None) == -2      # channel count without a kernel
    assert lib.eg_conv1d(one, one, one, one, None, one, 1, 4, 4, 8, 3, 1, 1, 1, None) == -1                    # scale without shift
    assert lib.eg_conv1d(one, one, one, None, None, one, 1, 4, 4, 2, 5, 1, 0, 0, None) == -1                   # kernel longer than the padded input
    assert lib.eg_contrastive_loss(one, one, 0, 4, None, one, one, one, 64, None) == -1                        # n = 0
    assert lib.eg_contrastive_loss(one, one, 8, 4, None, one, one, one, 8, None) == -3                         # workspace too small
    assert lib.eg_multi_head_attention(one, one, one, one, one, one, one, one, one, None, 1, 4, 4, 510, 8, 0, one, 1 << 30, None) == -2   # d_model % 4
    assert lib.eg_se_gate(one, 4, one, one, one, one, one, 1, 200, 16, None) == -2                              # C = 200
    assert lib.eg_generator_forward(None, None, 1, None, None, None, None, None, None, None, None, None, None, 0, None) < 0
    assert lib.eg_mel_workspace_bytes(0, 64000) == 0 and lib.eg_mel_workspace_bytes(2, 64000) == 2 * 128 * 126 * 4
    # the four entry points of kernels the generator and the CVAE launch internally (tests/misc_f64.py)
    with pytest.raises(_lib.EgError, match="chunk=65"):
        GeneratorEngine(variant="memory", frames=128, prior_frames=100, chunk=65)      # the TM scores live in 64 slots
    with pytest.raises(_lib.EgError, match="chunk=10"):
        GeneratorEngine(variant="memory", frames=34, prior_frames=30, chunk=10)        # only 4 predicted frames to gate
    conv, mem = (C.c_void_p * 8)(*[16] * 8), (C.c_void_p * 12)(*[16] * 12)
    none12, part = (C.c_void_p * 12)(), (C.c_void_p * 12)(*[16] * 11)
    pe = lambda cv, mm, *a: lib.eg_prior_encoder(one, cv, mm, one, one, one, one, *a, None)
    assert pe(conv, None, 2, 4, 34, 126, 125, 4, 0) == -1 and b"dpad=125 < d=126" in lib.eg_last_error()
    assert pe(conv, part, 2, 4, 34, 126, 128, 4, 1) == -1 and b"partly set (11 of 12)" in lib.eg_last_error()
    assert pe(conv, mem, 2, 4, 34, 126, 128, 4, 0) == -1 and pe(conv, none12, 2, 4, 34, 126, 128, 4, 1) == -1      # pointers against the variant
    assert pe(conv, mem, 2, 100, 128, 126, 128, 65, 1) == -1 and b"chunk=65" in lib.eg_last_error()
    assert pe(conv, mem, 2, 4, 34, 126, 128, 0, 1) == -1 and pe(conv, mem, 2, 4, 34, 126, 128, 5, 1) == -1           # chunk < 1, chunk > prior_frames
    assert pe(conv, mem, 2, 30, 34, 126, 128, 5, 1) == -1 and b"= 4" in lib.eg_last_error()                          # chunk > frames - prior_frames
    assert pe((C.c_void_p * 8)(*[16] * 7), None, 2, 4, 34, 126, 128, 4, 0) == -1 and b"conv[7]" in lib.eg_last_error()
    assert pe(conv, mem, 1, 10, 120, 282, 320, 10, 1) == -2 and b"LDS need" in lib.eg_last_error()                   # 181 KB for one workgroup
    assert lib.eg_embedding(one, one, one, None, None, 4, 6, 8, 10, None) == -5 and b"dim=6" in lib.eg_last_error()
    assert lib.eg_embedding(one, one, one, None, None, 4, 8, 4, 10, None) == -5 and b"ld=4 < dim=8" in lib.eg_last_error()
    assert lib.eg_embedding(one, one, one, one, None, 4, 8, 32, 10, None) == -5 and b"images need ld % 64 == 0" in lib.eg_last_error()
    assert lib.eg_embedding(one, one, one, None, one, 4, 8, 64, 10, None) == -1 and b"zero_line without images" in lib.eg_last_error()
    assert lib.eg_embedding(one, one, None, None, None, 4, 8, 64, 10, None) == -1 and lib.eg_embedding(one, one, one, None, None, 0, 8, 64, 10, None) == -1
    assert lib.eg_small_linear(one, 8, one, one, None, 16, 2, 8, 16, None) == -1                                      # null y
    assert lib.eg_small_linear(one, 7, one, one, one, 16, 2, 8, 16, None) == -1 and b"ldx=7" in lib.eg_last_error()   # ldx < in
    assert lib.eg_small_linear(one, 8, one, one, one, 15, 2, 8, 16, None) == -1 and lib.eg_small_linear(one, 8, one, one, one, 16, 0, 8, 16, None) == -1
    assert lib.eg_conv_transpose1d(one, one, one, None, None, one, 2, 4, 8, 16, None) == -1 and b"scale and shift are required" in lib.eg_last_error()
    assert lib.eg_conv_transpose1d(one, one, one, one, one, one, 2, 4, 8, 0, None) == -1 and b"lin=0" in lib.eg_last_error()


def test_conv_pack_layout_roundtrip():
    """EG_PACK_CONV3X3: fp32 image [tap][ci/4][co][4]; bf16 images hi + lo reconstruct the weight to ~2^-16."""
    from emotiongestures_amd import packing
    w = torch.randn(34, 128, 3, 3)
    p = packing._pack_conv3x3(w, 48)
    n32 = 9 * 128 * 48
    f32 = torch.from_numpy(p[:n32].copy()).view(9, 32, 48, 4)
    assert torch.equal(f32[4, 3, 7], w[7, 12:16, 1, 1])
    assert torch.all(f32[:, :, 34:] == 0)
    bits = p[n32:].view(np.int16)
    hi = torch.from_numpy(bits[: n32].copy()).view(torch.bfloat16).float().view(9, 16, 48, 8)
    lo = torch.from_numpy(bits[n32:].copy()).view(torch.bfloat16).float().view(9, 16, 48, 8)
    rec = (hi + lo)[2, 5, 11]                 # tap (0,2), ci 40..47, co 11
    assert torch.allclose(rec, w[11, 40:48, 0, 2], rtol=2 ** -15, atol=1e-7)


def test_shard_range_properties():
    from emotiongestures_amd.dist import shard_range
    for n in (0, 1, 7, 64, 1000):
        for world in (1, 2, 3, 8):
            spans = [shard_range(n, r, world) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            sizes = [e - b for b, e in spans]
            assert max(sizes) - min(sizes) <= 1
    with pytest.raises(ValueError):
        shard_range(4, 2, 2)


_WORKER = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from emotiongestures_amd.dist import shard_range, shard_batch, gather_poses, init_process_group
init_process_group("gloo", int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]))
rank, world = dist.get_rank(), dist.get_world_size()
n = 7
full = torch.arange(n * 34 * 126, dtype=torch.float32).view(n, 34, 126)
mine = shard_batch({"pose": full}, rank, world)["pose"]
out = gather_poses(mine * 1.0, n)
assert torch.equal(out, full), "gather mismatch"
dist.barrier(); dist.destroy_process_group()
print("ok", rank)
'''


def test_two_rank_gloo_shard_and_gather(tmp_path):
    """N>1 path on CPU: two gloo ranks shard 7 clips 4/3, run independently, and all-gather the ragged pose shards."""
    script = tmp_path / "w.py"
    script.write_text(_WORKER)
    env = dict(os.environ, EG_DIST_STORE=str(tmp_path / "store"), WORLD_SIZE="2")         # file rendezvous: no fixed or probed TCP port
    env.pop("MASTER_PORT", None)
    procs = [subprocess.Popen([sys.executable, str(script), ROOT], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT) for r in range(2)]
    outs = [p.communicate(timeout=240)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    assert all("ok" in o for o in outs)


def test_install_aliases_resolve_reference_import_lines():
    """The reference's own import lines (test_emotion_gesture_diversity_iterative.py:25-30 and the data path) resolve to the
    mirrors after install_aliases(); run in a child process so this session's sys.modules stays clean."""
    import subprocess
    import sys
    code = (
        "import emotiongestures_amd as E; E.install_aliases()\n"
        "from Full_model.Models_memory import Transformer, Motion_Discriminator\n"
        "from Full_model.Models_spatial_memory import Transformer as T2\n"
        "from CAVE.BEAT_CVAE import MLP_Reconstruct_v3 as VAE\n"
        "from model.FGD import MLP_Reconstruct\n"
        "from model.FHD_score import calculate_frechet_distance, diversity_score\n"
        "from skeleton_classifer.Models import Transformer as skeleton_header\n"
        "from model.audio_emotion_classifer import EmotionNet\n"
        "from model.motion_ae import MotionAE\n"
        "from model.embedding_space_evaluator import EmbeddingSpaceEvaluator\n"
        "from data_loader.data_preprocessor_expressive import DataPreprocessor\n"
        "from data_loader.lmdb_loader_BEAT_full import SpeechMotionDataset, one_hot_eid\n"
        "from utils.train_utils_BEAT import extract_melspectrogram, make_audio_fixed_length\n"
        # :29 -- the metric is out of scope (librosa), the import line and the caller's construction (:185) are not; its methods refuse loudly
        "from model.Beat_score_v2 import alignment\n"
        "al = alignment(0.3, 2)\n"
        "assert (al.sigma, al.order) == (0.3, 2)\n"
        "try:\n"
        "    al.load_audio(None, 0, True)\n"
        "    raise SystemExit('load_audio did not refuse')\n"
        "except NotImplementedError as e:\n"
        "    assert 'librosa' in str(e)\n"
        "print('ok')\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]


def test_pipeline_argument_validation_without_gpu():
    """ClipPipeline refuses a CPU device / bad lane counts before touching any engine (there is no CPU fallback)."""
    from emotiongestures_amd.pipeline import ClipPipeline
    with pytest.raises(ValueError):
        ClipPipeline((None, None, None), {}, "cuda:0", lanes=0)
    with pytest.raises(RuntimeError):
        ClipPipeline((None, None, None), {}, "cpu", lanes=2)


def test_launch_histogram_is_empty_unless_enabled_and_reports_its_size():
    """eg_launch_histogram (diagnostic): without EG_LAUNCH_HIST=1 nothing is counted -- the text is empty, the call returns the one byte of its NUL and
    tolerates a null / too small buffer; host-only, no GPU call."""
    import ctypes
    from emotiongestures_amd import _lib as L
    lib = L.load()
    if os.environ.get("EG_LAUNCH_HIST") == "1":
        pytest.skip("histogram enabled in this environment")
    assert int(lib.eg_launch_histogram(None, 0, 0)) == 1
    buf = ctypes.create_string_buffer(8)
    assert int(lib.eg_launch_histogram(buf, len(buf), 1)) == 1 and buf.value == b""
