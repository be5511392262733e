"""Test-side restatements for the motion-clip features of whole tracks (emotiongestures_amd.motionfeat, csrc/motionfeat.hip).  A helper module
(not collected: no test_ prefix); it runs on the CPU and imports nothing that touches a GPU.

  windows     the clip order restated from the definition (recording-major, then take, then window; the tail window last) and the windows
              cut on the host by plain indexing
  tower       PoseEncoderConv.net in float64 on fp32 inputs, with the a-priori fp32 bound of every element carried through the four layers
"""
import numpy as np
import torch
import torch.nn.functional as TF

U32 = 2.0 ** -24          # unit round-off of fp32
WINDOW = 34
TOWER = ((1, True), (1, True), (2, True), (1, False))      # (stride, LeakyReLU) of the four convolutions


def nan_track(U, R, Tmax, D, frames, seed, scale=0.8):
    """Uniform poses in [-scale, scale], every row at or beyond frames[u] NaN."""
    rng = np.random.default_rng(seed)
    trk = ((rng.random((U, R, Tmax, D)) * 2 - 1) * scale).astype(np.float32)
    for u, f in enumerate(frames):
        trk[u, :, f:] = np.nan
    return trk


def window_starts(f, stride, tail):
    s = list(range(0, f - WINDOW + 1, stride))
    if tail and (f - WINDOW) % stride:
        s.append(f - WINDOW)
    return s


def clip_list(frames, R, stride, tail):
    """[(u, r, start)] in clip order, from the definition."""
    return [(u, r, s) for u, f in enumerate(frames) for r in range(R) for s in window_starts(f, stride, tail)]


def cut_windows(track, frames, stride, tail):
    """track [U, R, Tmax, D] (numpy) -> [N, 34, D]: every window by plain indexing, in clip order."""
    clips = clip_list(frames, track.shape[1], stride, tail)
    return np.stack([track[u, r, s:s + WINDOW] for u, r, s in clips])


def tower_f64(windows, weights):
    """windows [N, 34, D] fp32 tensor, weights [(w [cout, cin, k], bias)] * 4 fp32 tensors -> (ref [N, 32, 12], bound [N, 32, 12]) float64.

    e_0 = 0;  e_l = (cin k + 4) u (|b| + |W| (|ref_{l-1}| + e_{l-1})) + |W| e_{l-1} + u |ref_l|:  the kernel adds the cin*k products to the bias
    one after the other in fp32 on inputs that are themselves e_{l-1} off (conv1d_bound of tests/small_ops_f64.py on the perturbed input),
    the input's error passes through |W|, LeakyReLU is 1-Lipschitz, and the last term is the rounding of the stored value."""
    x = windows.double().transpose(1, 2)
    e = torch.zeros_like(x)
    for (w, b), (stride, act) in zip(weights, TOWER):
        w, b = w.double().cpu(), b.double().cpu()
        cin, k = w.shape[1], w.shape[2]
        ref = TF.conv1d(x, w, b, stride=stride)
        if act:
            ref = TF.leaky_relu(ref, 0.2)
        mag = TF.conv1d(x.abs() + e, w.abs(), b.abs(), stride=stride)
        e = (cin * k + 4) * U32 * mag + TF.conv1d(e, w.abs(), None, stride=stride) + U32 * ref.abs()
        x = ref
    return x, e
