// csrc/avad_gain.h -- the loudness arithmetic of a prepared trial (Part 7 of include/dss_hip.h), the part that the kernels
// (acoustic_vad.hip) and the library's host checker (dss_avad.cpp) share word for word.
//
// The reference normalises every non-silence trial through pydub (prepare_corpus._normalize_audio, prepare_corpus.py:33-40):
// effects.normalize, then apply_gain(-3).  Each of the two is one audioop.mul over the int16 samples, which is
// floor(fbound(sample * factor)) in double with fbound clipping to [-32768, 32767] -- its lower test is `< -32767`, so
// everything below -32767 becomes -32768.  Two roundings, not one: the two gains must not be folded into one product.
// No fused multiply-add can arise (one product, nothing added), and the library is built with -ffp-contract=off.
#pragma once

#define AVAD_GAIN_ENTRIES 32769   // one factor per peak 0 .. 32768

// max |x| of one sample as int: -32768 counts as 32768
__host__ __device__ static inline int avad_abs16(short x)
{
    const int v = (int)x;
    return v < 0 ? -v : v;
}

// audioop.mul on one int16 sample
__host__ __device__ static inline short avad_scale(short x, double f)
{
    double v = (double)x * f;
    if (v > 32767.0) v = 32767.0;
    else if (v < -32767.0) v = -32768.0;
    return (short)(int)__builtin_floor(v);
}

// the prepared sample of a normalised trial: the factor of the trial's peak, then the post gain, each rounded on its own
__host__ __device__ static inline short avad_prepared(short x, double gain, double post)
{
    return avad_scale(avad_scale(x, gain), post);
}
