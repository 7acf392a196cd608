// csrc/lpc_tables.h -- the derived tables of lpc_from_cepstrum (host libm, exactly as xiph builds them at run time), for the two
// owners that upload them: the LPCNet model (dss_lpcnet_model.cpp) and the feature encoder (dss_fenc.cpp), which needs no model.
// Host code only.
#pragma once

#include <math.h>

#include <vector>

struct LpcTables {
    float dct[18 * 18], costab[320], ia[160], ib[160];
    int iband[160];
    double lagw[17];
    std::vector<float> cos_kl;       // [160][17]
    LpcTables()
    {
        for (int i = 0; i < 18; ++i)                                                                  // freq.c check_init()
            for (int j = 0; j < 18; ++j) {
                dct[i * 18 + j] = cos((i + .5) * j * M_PI / 18);
                if (j == 0) dct[i * 18 + j] *= sqrt(.5);
            }
        for (int i = 0; i < 320; ++i) costab[i] = (float)cos(2. * M_PI * i / 320);
        static const int eband5ms[18] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 24, 28, 34, 40};
        for (int i = 0; i < 17; ++i) {                                                                // interp_band_gain()
            const int band_size = (eband5ms[i + 1] - eband5ms[i]) * 4;
            for (int j = 0; j < band_size; ++j) {
                const float frac = (float)j / band_size;
                ia[eband5ms[i] * 4 + j] = 1 - frac;
                ib[eband5ms[i] * 4 + j] = frac;
                iband[eband5ms[i] * 4 + j] = i;
            }
        }
        for (int i = 0; i < 17; ++i) lagw[i] = (1 - 6e-5 * i * i);
        cos_kl.resize((size_t)160 * 17);
        for (int k = 0; k < 160; ++k)
            for (int lag = 0; lag < 17; ++lag) cos_kl[(size_t)k * 17 + lag] = costab[(k * lag) % 320];
    }
};
