// mlp_pack.hip -- host code every fused inference MLP family packs its weights with (declared in sa_mlp_common.h):
// the split of an fp32 weight into three bf16 levels, one 32x32 tile pair in the MFMA operand layout, a layer's bias
// in operand order, and the zero pairs that fill a stream up to a whole LDS stage. Plain C loops, no device work; the
// formulation these layouts serve is described in sa_mlp.hip.
#include "sa_mlp_common.h"

#include <string.h>

namespace pn2 {

static unsigned short bf16_nearest_even(float f)
{
    unsigned int u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40);      // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}

static float bf16_value(unsigned short b)
{
    const unsigned int u = (unsigned int)b << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

static void mlp_split_weight(float w, unsigned short out[3])
{
    out[0] = bf16_nearest_even(w);
    const float r1 = w - bf16_value(out[0]);              // exact: the residual of a nearest rounding fits in fp32
    out[1] = bf16_nearest_even(r1);
    const float r2 = r1 - bf16_value(out[1]);
    out[2] = bf16_nearest_even(r2);
}

// value for K16 step e, level, lane l, slot j = level of W[krow(32u + mlp_chan(8e + j, l >> 5))][32t + (l & 31)]
float *mlp_pack_pair_x6(float *wp, const float *w, int kin, int nout, int t, int u, const int *krow)
{
    unsigned short *o = reinterpret_cast<unsigned short *>(wp);
    for (int e = 0; e < 2; ++e)
        for (int lane = 0; lane < 64; ++lane)
            for (int j = 0; j < 8; ++j) {
                const int k = 32 * u + mlp_chan(8 * e + j, lane >> 5), nn = 32 * t + (lane & 31);
                const float val = (k < kin && nn < nout) ? w[(size_t)(krow ? krow[k] : k) * nout + nn] : 0.0f;
                unsigned short lv[3];
                mlp_split_weight(val, lv);
                for (int level = 0; level < 3; ++level) o[(((e * 3 + level) * 64 + lane) * 8) + j] = lv[level];
            }
    return wp + kPairWords;
}

float *mlp_pack_bias(float *bp, const float *bias, int nout, int tiles)
{
    for (int t = 0; t < tiles; ++t)
        for (int hh = 0; hh < 2; ++hh)
            for (int v = 0; v < 16; ++v) {
                const int ch = 32 * t + mlp_chan(v, hh);
                *bp++ = (bias && ch < nout) ? bias[ch] : 0.0f;
            }
    return bp;
}

float *mlp_pack_stage_padding(float *wp, int pairs)
{
    const size_t words = (size_t)(pad_to_stage(pairs) - pairs) * kPairWords;
    memset(wp, 0, sizeof(float) * words);
    return wp + words;
}

}  // namespace pn2
