"""Import-line mirror of model/Beat_score_v2.py so that `from model.Beat_score_v2 import alignment`
(test_emotion_gesture_diversity_iterative.py:29) resolves after `install_aliases()`.

This default is a refusing stub: `alignment(sigma, order)` constructs (the caller builds it before its loop, :185) and every method that would
compute something raises `BeatScoreUnavailable`, as do the two other metric classes of that file.  The metric itself lives in
`emotiongestures_amd.beat` (batched `beat_alignment` on the GPU, and a drop-in `alignment` class); `install_aliases(beat_score=True)` points
`model.Beat_score_v2` there.  It is opt-in because its audio half is restated from librosa 0.10's documented onset routines and is not
pinned against librosa itself."""


class BeatScoreUnavailable(NotImplementedError):
    pass


def _refuse(what):
    raise BeatScoreUnavailable(f"model.Beat_score_v2.{what}: the librosa-restated beat score is opt-in "
                               "(install_aliases(beat_score=True), or emotiongestures_amd.beat)")


class alignment(object):
    """model/Beat_score_v2.py:51-56: keeps (sigma, order) like upstream; see the module docstring."""

    def __init__(self, sigma, order):
        self.sigma = sigma
        self.order = order
        self.times = None
        self.oenv = None
        self.S = None
        self.rms = None
        self.pose_data = []

    def load_audio(self, *a, **k):
        _refuse("alignment.load_audio")

    def load_pose(self, *a, **k):
        _refuse("alignment.load_pose")

    def load_data(self, *a, **k):
        _refuse("alignment.load_data")

    def eval_random_pose(self, *a, **k):
        _refuse("alignment.eval_random_pose")

    def audio_beat_vis(self, *a, **k):
        _refuse("alignment.audio_beat_vis")

    def calculate_align(self, *a, **k):
        _refuse("alignment.calculate_align")


class L1div(object):
    def __init__(self, *a, **k):
        _refuse("L1div")


class SRGR(object):
    def __init__(self, *a, **k):
        _refuse("SRGR")
