"""Cases of the acoustic VAD kernels (csrc/acoustic_vad.hip) for the tests (helper module, no tests in it).

tests/golden/acoustic_vad.npz and the tests on it sit on one geometry: 16 kHz, a window of 800 samples every 160, 401 bins,
40 bands.  ``AcousticVadGPU`` takes others, and avad_energy_kernel takes other branches when it gets them: fewer than four
blocks of 16 bins (waves without a block), a k loop of one step, bands whose run of the mel matrix is empty, a band loop of one
pass or of two, the log-mel area that aliases the samples being the larger of the two, no overlap between frames, a shift of
one sample, and the last window and the last shift whose tile still fits LDS.  ``GEOMETRY`` names the smallest shapes that
reach each, ``REFUSALS`` the first shapes past the limits, ``EDGES`` the trial shapes at the default geometry that sit on the
32-frame tile, on the shift, on the lead and on the ends of the audio.

The geometry cases are held to tests/golden/acoustic_vad_cases.npz, which the reference's own EnergyBasedVad computed
(tools/make_golden_acoustic_vad.py); the edges to the float64 restatement in tests/acoustic_vad_reference.py.  The integers of
the table (N, shift, bins, nblk, empty bands, LDS bytes) are what a case is there to reach: tests/test_cpu_acoustic_vad_cases.py
computes them again from the package and the library and compares.

Bounds on the log energy are per case and come from the CPU alone (tools/acoustic_vad_bounds.py): D is the largest
|restatement - fixture| over the case's trials (pocketfft and BLAS against a direct DFT and a matmul: two independent float64
evaluations of which the kernel is a third), U one ulp of the case's largest |log energy|, and the bound 4 x max(D, U), the
margin tests/test_gpu_acoustic_vad.py gives a different summation order and a different log.  No bound may pass ``CAP``.
"""
from __future__ import annotations

import collections
import functools

import numpy as np

from dss_amd.synthetic import synthetic_speech_audio

TILE = 32                        # AVAD_TILE_FRAMES
MAX_BANDS = 64                   # AVAD_MAX_BANDS
LDS_LIMIT = 163840               # AVAD_LDS_LIMIT
GAP = 1e-6                       # no compared frame lies this close to its trial's threshold: 10^4 x CAP
CAP = 1e-10                      # no bound on the log energy may pass this
MARGIN = 4.0
# the default geometry's bound (tests/test_gpu_acoustic_vad.py): 4 x the restatement's deviation from the first fixture
LOG_ENERGY_BOUND = 4 * 7.96e-13

DEFAULT = (16000, 0.05, 0.01, 40)


def lds_bytes(N, shift, bins, bands):
    """dss_avad_energy_lds_bytes restated: the twiddles and the window (3 N doubles), TILE rows of magnitudes, and the larger
    of the tile's samples (ints) and its log-mel rows (doubles), rounded up to 16 bytes."""
    tail = max(((TILE - 1) * shift + N) * 4, TILE * bands * 8)
    return (3 * N + TILE * bins) * 8 + ((tail + 15) & ~15)


def nblk_of(bins):
    return (bins + 15) >> 4


# lds: bytes of the tile; empty: bands whose column of the mel matrix is all zero; D: max |restatement - fixture| over the
# case's four trials as tools/acoustic_vad_bounds.py measures it, rounded up to three digits (measured: 4.547e-13, 3.979e-13,
# 4.547e-13, 2.274e-13, 1.364e-12, 3.553e-15, 3.126e-13, 3.411e-13, 1.776e-15, 1.421e-14, 4.263e-14 in the table's order; the
# same on two CPUs, and with BLAS on one thread never larger).
Case = collections.namedtuple("Case", "name fs window_length frame_shift n_bands N shift bins nblk empty lds D note")

GEOMETRY = (
    Case("fs_8k", 8000, 0.05, 0.01, 40, 400, 80, 201, 13, 0, 72576, 4.55e-13,
         "the one parameter the reference itself varies"),
    Case("short_8k", 8000, 0.025, 0.005, 40, 200, 40, 101, 7, 0, 40896, 3.98e-13,
         "half the window at 8 kHz; log-mel rows (10240 B) larger than the samples (5760 B)"),
    Case("fs_48k", 48000, 0.015, 0.005, 40, 720, 240, 361, 23, 0, 142336, 4.55e-13, "48 kHz"),
    Case("no_overlap_64", 16000, 0.004, 0.004, 40, 64, 64, 33, 3, 14, 20224, 2.28e-13,
         "shift == window; nblk = 3, wave 3 owns no block; 14 empty bands"),
    Case("shift_1_bands_64", 16000, 0.004, 6.25e-05, 64, 64, 1, 33, 3, 33, 26368, 1.37e-12,
         "log-mel rows (16384 B) larger than the samples (380 B); 33 empty bands; AVAD_MAX_BANDS"),
    Case("window_4", 16000, 0.00025, 0.000125, 2, 4, 2, 3, 1, 0, 1376, 3.56e-15, "one k step; nblk = 1, three waves idle"),
    Case("last_window", 16000, 0.0575, 0.01, 40, 920, 160, 461, 29, 0, 163616, 3.13e-13,
         "the last window that fits at a shift of 160: 224 bytes under the limit"),
    Case("last_shift", 16000, 0.05, 0.0195, 40, 800, 312, 401, 26, 0, 163744, 3.42e-13,
         "the last shift that fits under a window of 800: 96 bytes under the limit"),
    Case("bands_1", 16000, 0.05, 0.01, 1, 800, 160, 401, 26, 0, 144896, 1.78e-15, "one band: 32 of 256 threads in the band loop"),
    Case("bands_8", 16000, 0.05, 0.01, 8, 800, 160, 401, 26, 0, 144896, 1.43e-14, "32 x 8 = 256: exactly one pass of the band loop"),
    Case("bands_9", 16000, 0.05, 0.01, 9, 800, 160, 401, 26, 0, 144896, 4.27e-14, "the first band count that needs a second pass"),
)
NAMES = tuple(c.name for c in GEOMETRY)

# avad_energy_kernel's worst |log energy - fixture| per case on an MI355X, as tests/test_gpu_acoustic_vad_cases.py printed it,
# beside the bound it was held to (4 x max(D, U)).  A record only: no test reads it and no bound was derived from it.
KERNEL_MEASURED = {
    "fs_8k": 5.116e-13,               # bound 1.820e-12
    "short_8k": 4.547e-13,            # bound 1.592e-12
    "fs_48k": 3.411e-13,              # bound 1.820e-12
    "no_overlap_64": 4.547e-13,       # bound 9.120e-13
    "shift_1_bands_64": 1.137e-12,    # bound 5.480e-12
    "window_4": 3.553e-15,            # bound 2.842e-14 (half an ulp: the bound is 4 U here)
    "last_window": 2.842e-13,         # bound 1.252e-12
    "last_shift": 2.558e-13,          # bound 1.368e-12
    "bands_1": 6.217e-15,             # bound 7.120e-15: 3.5 ulp of a log energy near -10, the one band sums all 401 bins
    "bands_8": 2.842e-14,             # bound 5.720e-14
    "bands_9": 4.263e-14,             # bound 1.708e-13
}
# the edge trials against the restatement on the same device: 2.274e-13 (speech, 494 frames) and 8.527e-14 (noise, 21 frames)
# under LOG_ENERGY_BOUND = 3.184e-12

# (changed parameters, N, shift, bands, LDS bytes or None, message): refused by dss_avad_check_params, no device needed
Refusal = collections.namedtuple("Refusal", "name fs window_length frame_shift n_bands N shift lds message")
REFUSALS = (
    Refusal("window_924", 16000, 0.05775, 0.01, 40, 924, 160, 164240, "does not fit the energy kernel's tile"),
    Refusal("shift_313", 16000, 0.05, 0.0195625, 40, 800, 313, 163872, "does not fit the energy kernel's tile"),
    Refusal("fs_22050", 22050, 0.05, 0.01, 40, 1102, 220, None, "multiple of 4"),
    Refusal("bands_65", 16000, 0.05, 0.01, 65, 800, 160, None, "mel bands"),
)


def case(name) -> Case:
    return GEOMETRY[NAMES.index(name)]


def geometry(fs, window_length, frame_shift):
    """(N, shift, bins) as AcousticVadGPU and the reference's from_wav derive them: int() of a float product."""
    N = int(fs * window_length)
    return N, int(fs * frame_shift), N // 2 + 1


def bound(name) -> float:
    """4 x max(D, U) of a case; U from the fixture's largest |log energy|, see ``ulp_of_largest``."""
    c = case(name)
    return MARGIN * max(c.D, U[name])


def ulp_of_largest(log_energy) -> float:
    return float(np.spacing(np.max(np.abs(log_energy))))


# one ulp of the largest |log energy| of each case's fixture frames (tools/acoustic_vad_bounds.py prints them)
U = {"fs_8k": 2.0 ** -44, "short_8k": 2.0 ** -44, "fs_48k": 2.0 ** -44, "no_overlap_64": 2.0 ** -43, "shift_1_bands_64": 2.0 ** -42,
     "window_4": 2.0 ** -47, "last_window": 2.0 ** -44, "last_shift": 2.0 ** -44, "bands_1": 2.0 ** -49, "bands_8": 2.0 ** -46,
     "bands_9": 2.0 ** -46}

# ---- trials of the geometry cases ---------------------------------------------------------------------------------------
TRIAL_FRAMES = (1, 32, 33, 71)
AUDIO_SECONDS = 4
# first sample of each of a case's four trials, as a fraction of the audio: moved until no frame lies within GAP of its
# trial's threshold (tools/make_golden_acoustic_vad.py asserts it); (0.05, 0.3, 0.55, 0.1) did for every case
FIRST_AT = {name: (0.05, 0.3, 0.55, 0.1) for name in NAMES}


def trial_lengths(N, shift):
    """W = 1, 32, 33 and 71: one window, a full tile, a tile and one frame with shift - 1 samples past the last frame, three
    tiles with one sample past it (none at a shift of 1, where one sample more is one frame more)."""
    return (N, N + 31 * shift, N + 32 * shift + shift - 1, N + 70 * shift + min(1, shift - 1))


def audio_seed(name):
    return 8600 + NAMES.index(name)


@functools.lru_cache(maxsize=None)
def audio(name):
    """The case's seeded int16 audio at its own sampling rate, read-only: broadband room noise and harmonic bursts (no pure
    tone, no DC: bins that cancel to rounding noise would sit beside the 1e-7 fuzz of the log)."""
    c = case(name)
    a = synthetic_speech_audio(audio_seed(name), AUDIO_SECONDS * c.fs, c.fs)
    a.setflags(write=False)
    return a


def trials(name):
    """[(first sample, length)] of a case, lead 0."""
    c = case(name)
    n = AUDIO_SECONDS * c.fs
    out = [(int(f * n), length) for f, length in zip(FIRST_AT[name], trial_lengths(c.N, c.shift))]
    assert all(a + b <= n for a, b in out), name
    return out


# ---- trial edges at the default geometry ---------------------------------------------------------------------------------
N0, SHIFT0 = 800, 160
EDGE_AUDIO_SAMPLES = 40000
NOISE_SAMPLES = 4000
TILE_SPAN = (TILE - 1) * SHIFT0 + N0          # samples one workgroup stages: 5760


@functools.lru_cache(maxsize=None)
def edge_audio(which):
    """"speech": seeded synthetic speech; "noise": full-scale white noise that holds both -32768 and 32767.  Read-only."""
    if which == "speech":
        a = synthetic_speech_audio(8650, EDGE_AUDIO_SAMPLES)
    else:
        a = np.random.default_rng(8651).integers(-32768, 32768, NOISE_SAMPLES).astype(np.int16)
        a[17], a[18] = -32768, 32767
        assert a.min() == -32768 and a.max() == 32767
    a.setflags(write=False)
    return a


def _len(W, past=0):
    return N0 + (W - 1) * SHIFT0 + past


Edge = collections.namedtuple("Edge", "name audio first length lead W")
EDGES = (
    # W on the 32-frame tile edge
    Edge("w_31", "speech", 3000, _len(31), 0, 31),
    Edge("w_32", "speech", 3100, _len(32), 0, 32),
    Edge("w_33", "speech", 3200, _len(33), 0, 33),
    Edge("w_64", "speech", 9000, _len(64), 0, 64),
    Edge("w_65", "speech", 9100, _len(65), 0, 65),
    # no multiple of the shift: 159 samples past the last frame
    Edge("past_159", "speech", 21001, _len(10, 159), 0, 10),
    # leads: 0 is every case above; 1, shift - 1, shift, shift + 1, a whole window
    Edge("lead_1", "speech", 15000, _len(12), 1, 12),
    Edge("lead_159", "speech", 15000, _len(12), 159, 12),
    Edge("lead_160", "speech", 15000, _len(12), 160, 12),
    Edge("lead_161", "speech", 15000, _len(12), 161, 12),
    Edge("lead_800", "speech", 15000, _len(12), 800, 12),
    # 32 shifts and 7 samples: every frame of the first tile but the last four lies in the zeros; and 7 samples more than the
    # first tile's whole span, so that its workgroup stages nothing but zeros
    Edge("lead_5127", "speech", 20000, _len(41), 32 * SHIFT0 + 7, 41),
    Edge("lead_tile_span", "speech", 20000, _len(41), TILE_SPAN + 7, 41),
    # nothing but the lead: no sample of the audio is read
    Edge("lead_whole", "speech", 12345, _len(5, 3), _len(5, 3), 5),
    Edge("lead_whole_at_end", "speech", EDGE_AUDIO_SAMPLES, _len(2), _len(2), 2),
    # the two ends of the audio
    Edge("from_sample_0", "speech", 0, _len(34, 1), 0, 34),
    Edge("to_last_sample", "speech", EDGE_AUDIO_SAMPLES - _len(33, 77), _len(33, 77), 0, 33),
    Edge("to_last_sample_led", "speech", EDGE_AUDIO_SAMPLES - _len(3) + 256, _len(3), 256, 3),
    # the same range twice in one list, with different leads
    Edge("twice_a", "speech", 27000, _len(20), 0, 20),
    Edge("twice_b", "speech", 27000, _len(20), 333, 20),
    # full scale: the whole noise, from its first sample to its last
    Edge("full_scale_noise", "noise", 0, NOISE_SAMPLES, 0, 21),
)
EDGE_NAMES = tuple(e.name for e in EDGES)


def edges(which):
    return tuple(e for e in EDGES if e.audio == which)


# ---- the exact vote ------------------------------------------------------------------------------------------------------
VOTE_FRAMES = (1, 2, 3, 9, 10, 11, 255, 256, 257, 700)      # around 2 context, and around the 256 strided sums
VOTE_CONTEXTS = (0, 1, 5, 8, 300)                           # 300: more than 257, under 700
VOTE_MEAN_SCALES = (0.0, 2.5)
VOTE_AUDIO_SAMPLES = 200000


@functools.lru_cache(maxsize=None)
def vote_audio():
    a = synthetic_speech_audio(8660, VOTE_AUDIO_SAMPLES)
    a.setflags(write=False)
    return a


def vote_trials():
    """One list of VOTE_FRAMES frames each, spread over the audio (they overlap, which the operator allows)."""
    out = [(1000 + 7919 * k, _len(W)) for k, W in enumerate(VOTE_FRAMES)]
    assert all(a + b <= VOTE_AUDIO_SAMPLES for a, b in out)
    return out


# ---- the exact invariances -----------------------------------------------------------------------------------------------
INVARIANCE_CASES = ("default", "no_overlap_64", "shift_1_bands_64")


def invariance_case(name):
    """-> (constructor arguments, N, shift, audio)."""
    if name == "default":
        return dict(zip(("fs", "window_length", "frame_shift", "n_bands"), DEFAULT)), N0, SHIFT0, edge_audio("speech")
    c = case(name)
    return dict(fs=c.fs, window_length=c.window_length, frame_shift=c.frame_shift, n_bands=c.n_bands), c.N, c.shift, audio(name)


def invariance_leads(N, shift):
    """1, shift +- 1, a window, and 7 more than a tile's span, without repeats or zeros."""
    span = (TILE - 1) * shift + N
    return tuple(sorted({L for L in (1, shift - 1, shift, shift + 1, N, span + 7) if L > 0}))
