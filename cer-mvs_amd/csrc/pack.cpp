// Host-side weight packing: every cer_*_pack entry point of include/cer_mvs.h with its size function, and the one copy of each primitive
// they share.  The kernel files keep kernel, argument struct and launcher; what packer and launcher must agree on is in pack.hpp.  Plain
// C++17 - no HIP header, nothing device-side: the Makefile compiles this file without an offload arch, and it builds as it stands under a host
// sanitizer.  The layout comments here are the packed formats' documentation.
#include "pack.hpp"
#include <math.h>
#include <string.h>
#include <vector>

namespace {

// ---------------------------------------------------------------------------------------------------------------- shared primitives

// A weight as two f16 halves: hi = f16(v), lo = f16((v - hi) * lo_scale).  lo_scale = 2^11 in the f16x3 and encoder layouts (the kernels undo
// it: lo stays a normal f16 for |v| down to 2^-14), 1 in the s16 layouts (their weights are pre-scaled towards 2^14).  Every packer clamps to
// the largest finite f16 first, except the stem's.
struct Split16 { _Float16 hi, lo; };
inline Split16 split16(float v, float lo_scale, bool clamp = true) {
    if (clamp) v = v > 65504.f ? 65504.f : (v < -65504.f ? -65504.f : v);
    const _Float16 hi = (_Float16)v;
    return {hi, (_Float16)((v - (float)hi) * lo_scale)};
}

// One k16-step of 32 output channels as the matrix instructions' weight fragment: hi plane | lo plane of [lane 64][8] halves each, lane
// (j = lane & 31, kg = lane >> 5) holding val(k = 8 kg + e, j), e = 0..7.  `plane` points at the hi plane: the step / plane index is the caller's.
template <class F>
void pack_slice(_Float16* plane, float lo_scale, F&& val, bool clamp = true) {
    for (int lane = 0; lane < 64; ++lane)
        for (int e = 0; e < 8; ++e) {
            const Split16 s = split16(val((lane >> 5) * 8 + e, lane & 31), lo_scale, clamp);
            plane[lane * 8 + e] = s.hi;
            plane[512 + lane * 8 + e] = s.lo;
        }
}

// One 32-channel step of the f16x3 and encoder layouts [step][ntile32][k16-step 2][hi|lo][lane][8], lo scaled by 2^11: val(k = 0..31, j)
template <class F>
void pack_step32(_Float16* packed, long step, int NT, int nt, F&& val) {
    for (int ks = 0; ks < 2; ++ks)
        pack_slice(packed + ((step * NT + nt) * 2 + ks) * 1024, 2048.0f, [&](int k, int j) { return val(ks * 16 + k, j); });
}

// e4m3 (OCP: bias 7, subnormals, no infinities, largest finite 448), round to nearest even, saturating
unsigned char e4m3(double v) {
    const unsigned sgn = v < 0 ? 0x80u : 0u;
    double a = fabs(v);
    if (!(a == a)) return 0x7f;
    if (a >= 448.0) return (unsigned char)(sgn | 0x7e);
    if (a < ldexp(1.0, -10)) return (unsigned char)sgn;    // below half the smallest subnormal (ties to even: 0)
    int e;
    frexp(a, &e);                                          // a = m * 2^e, m in [0.5, 1)
    int E = e - 1;                                         // a in [2^E, 2^(E+1))
    if (E < -6) E = -6;                                    // subnormal range: spacing 2^-9
    const double q = nearbyint(ldexp(a, 3 - E));           // in units of 2^(E-3) (nearbyint: ties to even in the default mode)
    int M = (int)q;                                        // 8..16 for normals, 0..8 for subnormals
    int Eb = E + 7;
    if (a < ldexp(1.0, -6)) { Eb = 0; if (M == 8) { Eb = 1; M = 0; } }
    else { if (M == 16) { M = 0; ++Eb; } else M -= 8; }
    if (Eb > 15 || (Eb == 15 && M > 6)) return (unsigned char)(sgn | 0x7e);
    return (unsigned char)(sgn | (Eb << 3) | M);
}

// e2m3 (FP6: 1 sign, 2 exponent, 3 mantissa bits: 0, 0.125 .. 0.875, 1 .. 1.875, 2 .. 3.75, 4 .. 7.5), round to nearest even, saturating
unsigned e2m3(double v) {
    const unsigned sgn = v < 0 ? 32u : 0u;
    const double a = fabs(v);
    if (!(a == a) || a >= 7.5) return sgn | 31u;
    const int E = a < 2.0 ? 0 : (a < 4.0 ? 1 : 2);          // steps of 0.125 (subnormals and [1, 2)), 0.25, 0.5
    const int q = (int)nearbyint(ldexp(a, 3 - E));          // a in units of the step: 0..16 (E = 0), 8..16
    if (E == 0) return sgn | (unsigned)q;                   // codes 0..15 are linear in the value (q = 16: code 16 = 2.0)
    return sgn | (unsigned)(8 * E + q);                     // e = E + 1, m = q - 8 (q = 16 carries into the next exponent: 7.5 is the cap above)
}

// One lane's K block of v_mfma_scale_f32_32x32x64_f8f6f4 in its FP6 form: the 32 values f, all divided by ONE power of two t = 2^(e - 2) (e:
// exponent of the block's largest magnitude; one up where that would land above 7.75), as six-bit e2m3 fields, field i at bit 6 i = dwords
// 0-5 (24 bytes); byte 24 = E8M0 of t * 2^-11 (the lane's scale operand), bytes 25-31 zero.  f = [wl * 2^11 (8) | wh (8)] of the chunk's first
// 16 channels, then of its second: the 2^-11 in the scale byte undoes the 2^11 on BOTH correction terms (the activations carry
// [xh | xl * 2^11] in the same positions).  An all-zero block takes t = 2^-100 (byte 16).
void fp6_block(const double f[32], unsigned q[8]) {
    double mx = 0.0;
    for (int i = 0; i < 32; ++i) mx = fmax(mx, fabs(f[i]));
    int te = -100;                                           // t = 2^te
    if (mx > 0.0) {
        int e2;
        frexp(mx, &e2);                                      // mx in [2^(e2-1), 2^e2)
        te = e2 - 1 - 2;
        if (ldexp(mx, -te) > 7.75) ++te;
        if (te < -100) te = -100;
    }
    memset(q, 0, 8 * sizeof(unsigned));
    for (int i = 0; i < 32; ++i) {
        const unsigned fld = e2m3(ldexp(f[i], -te));
        const int bit = 6 * i;
        q[bit >> 5] |= fld << (bit & 31);
        if ((bit & 31) > 26) q[(bit >> 5) + 1] |= fld >> (32 - (bit & 31));
    }
    q[6] = (unsigned)(te - 11 + 127);
}

// FP6-correction form of one 32-channel step of 32 output channels, val(k = 0..31, j): two hi planes ([lane][8] halves as in pack_slice, of
// channels 0-15 and 16-31) and, per lane, the two 16-byte halves of its fp6_block (lane (j, kg): channels 8 kg .. 8 kg + 7 of either half) in
// q0 and q1.  Where the four planes lie is the caller's layout.
template <class F>
void pack_chunk6(_Float16* hi0, _Float16* hi1, char* q0, char* q1, float lo_scale, F&& val) {
    for (int lane = 0; lane < 64; ++lane) {
        double f[32];
        for (int hc = 0; hc < 2; ++hc)
            for (int e = 0; e < 8; ++e) {
                const Split16 s = split16(val(hc * 16 + (lane >> 5) * 8 + e, lane & 31), lo_scale);
                (hc ? hi1 : hi0)[lane * 8 + e] = s.hi;
                f[hc * 16 + e] = (double)(float)s.lo * (2048.0f / lo_scale);
                f[hc * 16 + 8 + e] = (double)(float)s.hi;
            }
        unsigned q[8];
        fp6_block(f, q);
        memcpy(q0 + lane * 16, q, 16);
        memcpy(q1 + lane * 16, q + 4, 16);
    }
}

// The collapsed 81-tap filter of a disparity source (49 unfold channels from c0) in fp64:
//   W9[co][s] = sum_{t + u = s} w[co][u][t]  -  [|s - 4| <= 1] * sum_u w[co][u][t = s - 3]
// (t over the 3x3 conv taps, u over the 7x7 unfold offsets, s = sidx over the 9x9 window; the second term is the centre subtraction of
// core/update.py:84).  Valid for pixels whose 3x3 neighbourhood lies inside the image.  sidx >= 81: padding, zero.
double w9(const float* w, int Cin, int co, int c0, int sidx) {
    if (sidx >= 81) return 0.0;
    const int sy = sidx / 9, sx = sidx % 9;
    double acc = 0.0;
    for (int ty = 0; ty < 3; ++ty)
        for (int tx = 0; tx < 3; ++tx) {
            const int uy = sy - ty, ux = sx - tx;
            if (uy >= 0 && uy < 7 && ux >= 0 && ux < 7) acc += (double)w[((long)co * Cin + c0 + uy * 7 + ux) * 9 + ty * 3 + tx];
        }
    if (sy >= 3 && sy <= 5 && sx >= 3 && sx <= 5) {
        const int t = (sy - 3) * 3 + (sx - 3);
        for (int u = 0; u < 49; ++u) acc -= (double)w[((long)co * Cin + c0 + u) * 9 + t];
    }
    return acc;
}

// fp32 and f16x3 update-block packs: argument checks, and padded K index -> real input channel (or -1)
int check_sources(const void* w, const void* packed, int Cout, int cout_multiple, int Cin, const int* ch, const int* kind, int nsrc) {
    if (!w || !packed || !ch || !kind || nsrc <= 0 || nsrc > CER_CONV_MAX_SRC) return CER_EINVAL;
    if (Cout % cout_multiple) return CER_ESHAPE;
    int real = 0;
    for (int s = 0; s < nsrc; ++s) {
        if (kind[s] == 1 && ch[s] != 49) return CER_ESHAPE;
        real += ch[s];
    }
    return real == Cin ? CER_OK : CER_ESHAPE;
}

std::vector<int> padded_map(const int* ch, const int* kind, int nsrc) {
    std::vector<int> map;
    int c = 0;
    for (int s = 0; s < nsrc; ++s) {
        const int pc = padded_channels(ch[s], kind[s]);
        for (int i = 0; i < pc; ++i) map.push_back(i < ch[s] ? c + i : -1);
        c += ch[s];
    }
    return map;
}

// Delta head projections: w2 OIHW [1, C, 3, 3] * 2^log2s -> [k16-step C/16][hi|lo][lane][8]: lane (tap = lane & 31, kg = lane >> 5) holds channels
// 16 step + 8 kg + e (tap >= 9: zero)
void pack_delta_proj(const float* w2, _Float16* packed, int C, float lo_scale, int log2s) {
    for (int step = 0; step < C / 16; ++step)
        pack_slice(packed + step * 1024L, lo_scale,
                   [&](int k, int tap) { return tap < 9 ? (float)ldexp((double)w2[(long)(step * 16 + k) * 9 + tap], log2s) : 0.f; });
}

}  // namespace

// ------------------------------------------------------------------------------------------------ fp32 update-block convs (gru.hip)

extern "C" long cer_conv3x3_packed_size(int Cout, int Kpad) {
    if (Cout <= 0 || Kpad <= 0 || Cout % 16 || Kpad % 16) return CER_ESHAPE;
    return (long)(Kpad / 16) * 9 * (Cout / 16) * 256;
}

// OIHW fp32 -> [chunk16][tap][ntile16][lane][4] floats: the B operands of v_mfma_f32_16x16x4_f32, lane (co = lane & 15, k = 4 (lane >> 4) + s4).
// Not the [lane][8] halves fragment of the other packs: its loop stays explicit.
extern "C" int cer_conv3x3_pack_f32(const float* w, float* packed, int Cout, int Cin, const int* ch, const int* kind, int nsrc) {
    if (const int rc = check_sources(w, packed, Cout, 16, Cin, ch, kind, nsrc)) return rc;
    const std::vector<int> map = padded_map(ch, kind, nsrc);
    const int NT = Cout / 16, KC = (int)map.size() / 16;
    for (int kc = 0; kc < KC; ++kc)
        for (int tap = 0; tap < 9; ++tap)
            for (int nt = 0; nt < NT; ++nt)
                for (int lane = 0; lane < 64; ++lane)
                    for (int s4 = 0; s4 < 4; ++s4) {
                        const int co = nt * 16 + (lane & 15);
                        const int ci = map[kc * 16 + (lane >> 4) * 4 + s4];
                        const float v = ci < 0 ? 0.f : w[((long)co * Cin + ci) * 9 + tap];
                        packed[((((long)kc * 9 + tap) * NT + nt) * 64 + lane) * 4 + s4] = v;
                    }
    return CER_OK;
}

// ------------------------------------------------------------------------------------------- f16x3 update-block convs (gru_f16x3.hip)

extern "C" long cer_conv3x3_f16x3_packed_size(int Cout, int Kpad) {
    if (Cout <= 0 || Kpad <= 0 || Cout % 32 || Kpad % 32) return CER_ESHAPE;
    return (long)(Kpad / 32) * 9 * (Cout / 32) * 2048;     // in halves (2 bytes each)
}

// OIHW fp32 -> [chunk32][tap][ntile32][k16-step][hi|lo][lane][8] halves, lo scaled by 2^11
extern "C" int cer_conv3x3_f16x3_pack(const float* w, void* packed_v, int Cout, int Cin, const int* ch, const int* kind, int nsrc) {
    if (const int rc = check_sources(w, packed_v, Cout, 32, Cin, ch, kind, nsrc)) return rc;
    const std::vector<int> map = padded_map(ch, kind, nsrc);
    const int NT = Cout / 32, KC = (int)map.size() / 32;
    for (int kc = 0; kc < KC; ++kc)
        for (int tap = 0; tap < 9; ++tap)
            for (int nt = 0; nt < NT; ++nt)
                pack_step32((_Float16*)packed_v, kc * 9 + tap, NT, nt, [&](int k, int j) {
                    const int ci = map[kc * 32 + k];
                    return ci < 0 ? 0.f : w[((long)(nt * 32 + j) * Cin + ci) * 9 + tap];
                });
    return CER_OK;
}

// Collapsed packing: same step order as above, except that a kind-1 (disparity) source contributes 3 single-tap steps holding the 81-tap
// filter w9 (rounded to fp32 before the split).
extern "C" long cer_conv3x3_f16x3_collapsed_size(int Cout, const int* ch, const int* kind, int nsrc) {
    if (!ch || !kind || nsrc <= 0 || nsrc > CER_CONV_MAX_SRC || Cout <= 0 || Cout % 32) return CER_ESHAPE;
    long steps = 0;
    for (int s = 0; s < nsrc; ++s) steps += kind[s] == 1 ? 3 : (padded_channels(ch[s], kind[s]) / 32) * 9;
    return steps * (Cout / 32) * 2048;
}

extern "C" int cer_conv3x3_f16x3_pack_collapsed(const float* w, void* packed_v, int Cout, int Cin, const int* ch, const int* kind, int nsrc) {
    if (const int rc = check_sources(w, packed_v, Cout, 32, Cin, ch, kind, nsrc)) return rc;
    _Float16* packed = (_Float16*)packed_v;
    const int NT = Cout / 32;
    long step = 0;
    int c = 0;
    for (int s = 0; s < nsrc; c += ch[s], ++s) {
        if (kind[s] == 1) {
            for (int kc = 0; kc < 3; ++kc, ++step)
                for (int nt = 0; nt < NT; ++nt)
                    pack_step32(packed, step, NT, nt, [&](int k, int j) { return (float)w9(w, Cin, nt * 32 + j, c, kc * 32 + k); });
        } else {
            for (int kc = 0; kc < padded_channels(ch[s], kind[s]) / 32; ++kc)
                for (int tap = 0; tap < 9; ++tap, ++step)
                    for (int nt = 0; nt < NT; ++nt)
                        pack_step32(packed, step, NT, nt, [&](int k, int j) {
                            const int ci = kc * 32 + k;
                            return ci < ch[s] ? w[((long)(nt * 32 + j) * Cin + c + ci) * 9 + tap] : 0.f;
                        });
        }
    }
    return CER_OK;
}

// delta head tail of the fused path: the B fragments of the [C x 9 (padded to 32)] projection, per 128-channel half 8 k16-steps
// (pack_delta_proj), lo scaled by 2^11
extern "C" long cer_delta_proj_packed_size(int C) { return C % 128 ? CER_ESHAPE : (long)(C / 128) * 8 * 2 * 512; }

extern "C" int cer_delta_proj_pack(const float* w2, void* packed_v, int C) {
    if (!w2 || !packed_v) return CER_EINVAL;
    if (C % 128) return CER_ESHAPE;
    pack_delta_proj(w2, (_Float16*)packed_v, C, 2048.0f, 0);
    return CER_OK;
}

// ------------------------------------------------------------------------------------------------ s16 update-block convs (conv_s16.hip)

extern "C" long cer_conv3x3_s16_packed_size(int Cout, const int* ch, const int* kind, int nsrc, int collapsed) {
    if (!ch || !kind || nsrc <= 0 || nsrc > CER_CONV_MAX_SRC || Cout <= 0 || Cout % 32) return CER_ESHAPE;
    int nd = 0;
    for (int s = 0; s < nsrc; ++s) {
        if (kind[s] == 1) { ++nd; if (ch[s] != 49) return CER_ESHAPE; }
        else if (ch[s] % 32) return CER_ESHAPE;
    }
    collapsed &= 1;                                        // (bit 1 = fp8-, bit 2 = FP6-correction form: same size)
    if (nd > 1 || (collapsed && nd == 0)) return CER_ESHAPE;
    long steps = 0;                                        // k16-steps: see cer_conv3x3_s16_pack
    for (int s = 0; s < nsrc; ++s) steps += kind[s] == 1 ? (collapsed ? 6 : 36) : (ch[s] / 16) * 9;
    return steps * (Cout / 32) * 1024;                     // in halves
}

// log2 of the product scale S shared by all sources: the largest power of two that keeps every scaled weight
// |w| * S / 2^log2sx(src) below 2^14 (f16 max 65504), for the literal and the collapsed packing alike.  Returns CER_ESHAPE
// (as a value < -1000) if some source's largest scaled weight would then fall below 2^-3 (its lo halves go subnormal: fewer than 22 bits).
extern "C" int cer_conv3x3_s16_scale(const float* w, int Cout, int Cin, const int* ch, const int* kind, const int* log2sx, int nsrc) {
    if (!w || !ch || !kind || !log2sx || nsrc <= 0 || nsrc > CER_CONV_MAX_SRC) return -100000;
    int c = 0;
    for (int s = 0; s < nsrc; ++s) c += ch[s];
    if (c != Cin) return -100000;                          // (before the scan: its reads are in bounds only if the sources add up to Cin)
    double wmax[CER_CONV_MAX_SRC];
    c = 0;
    for (int s = 0; s < nsrc; ++s) {
        double m = 0.0;
        for (int co = 0; co < Cout; ++co) {
            for (int i = 0; i < ch[s]; ++i)
                for (int t = 0; t < 9; ++t) m = fmax(m, fabs((double)w[((long)co * Cin + c + i) * 9 + t]));
            if (kind[s] == 1) {
                for (int sidx = 0; sidx < 81; ++sidx) m = fmax(m, fabs(w9(w, Cin, co, c, sidx)));
                // the rim-correction filters sum at most 3 taps per entry
                double m3 = 0.0;
                for (int u = 0; u < 49; ++u) {
                    for (int ty = 0; ty < 3; ++ty) {
                        double sr = 0.0;
                        for (int tx = 0; tx < 3; ++tx) sr += fabs((double)w[((long)co * Cin + c + u) * 9 + ty * 3 + tx]);
                        m3 = fmax(m3, sr);
                    }
                    for (int tx = 0; tx < 3; ++tx) {
                        double sc = 0.0;
                        for (int ty = 0; ty < 3; ++ty) sc += fabs((double)w[((long)co * Cin + c + u) * 9 + ty * 3 + tx]);
                        m3 = fmax(m3, sc);
                    }
                }
                m = fmax(m, m3);
            }
        }
        wmax[s] = m;
        c += ch[s];
    }
    int best = 1000;
    for (int s = 0; s < nsrc; ++s) {
        if (wmax[s] <= 0.0) continue;
        const int k = (int)floor(log2(16384.0 / wmax[s])) + log2sx[s];
        best = k < best ? k : best;
    }
    if (best == 1000) best = 14;
    // the shared scale is set by the source with the largest weights.  A source's lo halves are f16 residuals of magnitude <= 2^-11 of
    // its scaled weights; once they fall into the f16 subnormal range (spacing 2^-24) the source keeps fewer than 22 bits relative to
    // its own largest weight when that weight, scaled, is below 2^-3: refuse, the caller falls back to the f16x3 kernels (per-tensor splits)
    for (int s = 0; s < nsrc; ++s)
        if (wmax[s] > 0.0 && ldexp(wmax[s], best - log2sx[s]) < 0.125) return -100000 + CER_ESHAPE;
    return best;
}

// Rim-correction filters of the collapsed disparity form (see the kernel's epilogue), packed like weight slices:
// [edge 8][k16-step 2][ntile][hi|lo][lane][8] halves of  -sign * Wedge[k][co] * 2^(log2S - log2sx(disparity source)):
// edges 0-3 = top, bottom, left, right (27 taps: top/bottom k = a * 9 + sx, left/right k = sy * 3 + b), 4-7 = the corner taps two
// edges share (9 taps, k = i * 3 + j; opposite sign): top-left, top-right, bottom-left, bottom-right.
extern "C" long cer_conv3x3_s16_edge_size(int Cout) { return (Cout > 0 && Cout % 32 == 0) ? 16L * (Cout / 32) * 1024 : CER_ESHAPE; }

extern "C" int cer_conv3x3_s16_edge_pack(const float* w, void* out_v, int Cout, int Cin, const int* ch, const int* kind, const int* log2sx, int nsrc,
                                         int log2S) {
    if (!w || !out_v || !ch || !kind || !log2sx || nsrc <= 0 || nsrc > CER_CONV_MAX_SRC) return CER_EINVAL;
    if (Cout % 32) return CER_ESHAPE;
    int c0 = -1, c = 0, sd = -1;
    for (int s = 0; s < nsrc; ++s) {
        if (kind[s] == 1) { if (ch[s] != 49 || c0 >= 0) return CER_ESHAPE; c0 = c; sd = s; }
        c += ch[s];
    }
    if (c != Cin || c0 < 0) return CER_ESHAPE;
    auto W = [&](int co, int uy, int ux, int ty, int tx) -> double {
        if (uy < 0 || uy > 6 || ux < 0 || ux > 6) return 0.0;
        return (double)w[((long)co * Cin + c0 + uy * 7 + ux) * 9 + ty * 3 + tx];
    };
    // Wedge[edge][k][co]
    auto edge_w = [&](int e, int k, int co) -> double {
        if (e < 4) {
            if (k >= 27) return 0.0;
            double v = 0;
            if (e == 0) { const int a = k / 9, sx = k % 9; for (int tx = 0; tx < 3; ++tx) v += W(co, a + 4, sx - tx, 0, tx); }
            if (e == 1) { const int a = k / 9, sx = k % 9; for (int tx = 0; tx < 3; ++tx) v += W(co, a, sx - tx, 2, tx); }
            if (e == 2) { const int sy = k / 3, b = k % 3; for (int ty = 0; ty < 3; ++ty) v += W(co, sy - ty, b + 4, ty, 0); }
            if (e == 3) { const int sy = k / 3, b = k % 3; for (int ty = 0; ty < 3; ++ty) v += W(co, sy - ty, b, ty, 2); }
            return -v;                                     // the rim terms are SUBTRACTED from the collapsed result
        }
        if (k >= 9) return 0.0;
        const int i = k / 3, j = k % 3;
        if (e == 4) return W(co, i + 4, j + 4, 0, 0);      // ... and the shared corner tap is added back once
        if (e == 5) return W(co, i + 4, j, 0, 2);
        if (e == 6) return W(co, i, j + 4, 2, 0);
        return W(co, i, j, 2, 2);
    };
    const int NT = Cout / 32;
    const double scale = ldexp(1.0, log2S - log2sx[sd]);
    for (int step = 0; step < 16; ++step)                  // (edge, k16-step)
        for (int nt = 0; nt < NT; ++nt)
            pack_slice((_Float16*)out_v + ((long)step * NT + nt) * 1024, 1.0f,
                       [&](int k, int j) { return (float)(edge_w(step >> 1, (step & 1) * 16 + k, nt * 32 + j) * scale); });
    return CER_OK;
}

// OIHW fp32 -> [step][ntile32][hi|lo][lane][8] halves of w * 2^(log2S - log2sx(src)) (the fp64 product rounded to fp32, then split; plain lo);
// steps: tensors in source order (32-channel chunk, 16-channel half, tap), then the disparity source (collapsed: 6 single-tap groups of the
// 81-tap filter w9; literal: 4 groups x 9 taps of the 49 unfold channels).
// collapsed & 2, the fp8-correction form of the tensor sources: a chunk step (32 channels, one tap) is 4 KiB per n-tile = f16 hi halves of
// half-chunk 0 | of half-chunk 1 (each [lane][8], as in pack_slice) | the A operand of v_mfma_scale_f32_32x32x64_f8f6f4, bytes 0-15 | bytes
// 16-31 of every lane: lane (co = lane & 31, kg = lane >> 5): e4m3 [wl * 2^5 (8) | wh * 2^-6 (8)] of half-chunk 0's channels 8kg..8kg+7,
// then the same of half-chunk 1.
// collapsed & 4, the FP6-correction form: the same 4 KiB with the lane's fp6_block in place of the e4m3 bytes (pack_chunk6).
extern "C" int cer_conv3x3_s16_pack(const float* w, void* packed_v, int Cout, int Cin, const int* ch, const int* kind, const int* log2sx,
                                    int nsrc, int collapsed, int log2S) {
    if (!w || !packed_v || !ch || !kind || !log2sx) return CER_EINVAL;
    if ((collapsed & 6) == 6) return CER_EINVAL;
    const int fp6 = (collapsed & 4) != 0;                   // tensor sources in the FP6-correction form (CER_EPI_CORR_FP6 launches)
    const int fp8 = (collapsed & 2) != 0 || fp6;            // ... in the fp8-correction form (CER_EPI_CORR_FP8 launches): same step structure
    collapsed &= 1;
    if (cer_conv3x3_s16_packed_size(Cout, ch, kind, nsrc, collapsed) < 0) return CER_ESHAPE;
    int order[CER_CONV_MAX_SRC], c0[CER_CONV_MAX_SRC];
    sx_order(kind, nsrc, order);
    int c = 0;
    for (int s = 0; s < nsrc; ++s) { c0[s] = c; c += ch[s]; }
    if (c != Cin) return CER_ESHAPE;
    _Float16* packed = (_Float16*)packed_v;
    const int NT = Cout / 32;
    long step = 0;
    for (int oi = 0; oi < nsrc; ++oi) {
        const int s = order[oi];
        const double scale = ldexp(1.0, log2S - log2sx[s]);
        auto wt = [&](int co, int ci, int tap) -> double { return w[((long)co * Cin + c0[s] + ci) * 9 + tap]; };
        auto slices = [&](auto&& val) {                     // k16-step `step` of every n-tile from the fp64 val(k, co)
            for (int nt = 0; nt < NT; ++nt)
                pack_slice(packed + (step * NT + nt) * 1024, 1.0f, [&](int k, int j) { return (float)(val(k, nt * 32 + j) * scale); });
        };
        if (kind[s] != 1 && fp8) {
            for (int c32 = 0; c32 < ch[s] / 32; ++c32)
                for (int tap = 0; tap < 9; ++tap, step += 2)
                    for (int nt = 0; nt < NT; ++nt) {
                        _Float16* hi = packed + (step / 2 * NT + nt) * 2048;
                        char* q = reinterpret_cast<char*>(hi + 1024);
                        auto val = [&](int k, int j) { return (float)(wt(nt * 32 + j, c32 * 32 + k, tap) * scale); };
                        if (fp6) { pack_chunk6(hi, hi + 512, q, q + 1024, 1.0f, val); continue; }
                        for (int lane = 0; lane < 64; ++lane)
                            for (int hc = 0; hc < 2; ++hc)
                                for (int e = 0; e < 8; ++e) {
                                    const Split16 v = split16(val(hc * 16 + (lane >> 5) * 8 + e, lane & 31), 1.0f);
                                    hi[hc * 512 + lane * 8 + e] = v.hi;
                                    unsigned char* b = reinterpret_cast<unsigned char*>(q + hc * 1024 + lane * 16);
                                    b[e] = e4m3(ldexp((double)(float)v.lo, 5));
                                    b[8 + e] = e4m3(ldexp((double)(float)v.hi, -6));
                                }
                    }
        } else if (kind[s] != 1) {
            for (int g = 0; g < ch[s] / 16; ++g)
                for (int tap = 0; tap < 9; ++tap, ++step) slices([&](int k, int co) { return wt(co, g * 16 + k, tap); });
        } else if (collapsed) {
            for (int g = 0; g < 6; ++g, ++step) slices([&](int k, int co) { return w9(w, Cin, co, c0[s], g * 16 + k); });
        } else {
            for (int g = 0; g < 4; ++g)
                for (int tap = 0; tap < 9; ++tap, ++step) slices([&](int k, int co) { return g * 16 + k < 49 ? wt(co, g * 16 + k, tap) : 0.0; });
        }
    }
    return CER_OK;
}

// delta head projection: the A fragments [C/32][k16-step 2] (pack_delta_proj) of w2 * 2^log2s, plain lo; *log2s_out = the scale applied
extern "C" long cer_delta_proj_s16_packed_size(int C) { return C % 128 ? CER_ESHAPE : (long)(C / 32) * 2 * 2 * 512; }

extern "C" int cer_delta_proj_s16_pack(const float* w2, void* packed_v, int C, int* log2s_out) {
    if (!w2 || !packed_v || !log2s_out) return CER_EINVAL;
    if (C % 128) return CER_ESHAPE;
    double m = 0.0;
    for (long i = 0; i < (long)C * 9; ++i) m = fmax(m, fabs((double)w2[i]));
    *log2s_out = m > 0.0 ? (int)floor(log2(16384.0 / m)) : 14;
    pack_delta_proj(w2, (_Float16*)packed_v, C, 1.0f, *log2s_out);
    return CER_OK;
}

// ------------------------------------------------------------------------------------------------- encoder convs (enc_conv.hip, enc_pc.hip)

// generic weight packing: OIHW [Cout, Cin, k, k] (k = 1 or 3) -> [chunk32][tap][ntile32][k16-step][hi|lo][lane][8]
extern "C" long cer_enc_conv_packed_size(int Cout, int Cin, int taps) {
    if (Cout <= 0 || Cin <= 0 || Cout % 32 || Cin % 32 || (taps != 1 && taps != 9)) return CER_ESHAPE;
    return (long)(Cin / 32) * taps * (Cout / 32) * 2048;
}

extern "C" int cer_enc_conv_pack(const float* w, void* packed_v, int Cout, int Cin, int taps) {
    if (!w || !packed_v) return CER_EINVAL;
    if (Cout % 32 || Cin % 32 || (taps != 1 && taps != 9)) return CER_ESHAPE;
    const int NT = Cout / 32;
    for (int kc = 0; kc < Cin / 32; ++kc)
        for (int tap = 0; tap < taps; ++tap)
            for (int nt = 0; nt < NT; ++nt)
                pack_step32((_Float16*)packed_v, kc * taps + tap, NT, nt,
                            [&](int k, int j) { return w[((long)(nt * 32 + j) * Cin + kc * 32 + k) * taps + tap]; });
    return CER_OK;
}

// Weights of the FP6-correction form: cer_enc_conv_pack's order and size, [chunk32][tap][ntile32][k16-step][hi | q][lane][16 B]: the hi planes as
// before; the q planes of a tap's two steps hold the lane's fp6_block (wl' = (w - wh) 2^11 as the lo planes carry it): dwords 0-3 in step 0's
// q plane, dwords 4-5 | E8M0 byte | 0 in step 1's.
extern "C" int cer_enc_conv_pack_f6(const float* w, void* packed_v, int Cout, int Cin, int taps) {
    if (!w || !packed_v) return CER_EINVAL;
    if (Cout % 32 || Cin % 32 || (taps != 1 && taps != 9)) return CER_ESHAPE;
    const int NT = Cout / 32;
    for (int kc = 0; kc < Cin / 32; ++kc)
        for (int tap = 0; tap < taps; ++tap)
            for (int nt = 0; nt < NT; ++nt) {
                _Float16* p = (_Float16*)packed_v + (((long)kc * taps + tap) * NT + nt) * 2048;       // 512-half planes: (ks 0: hi, q), (ks 1: hi, q)
                pack_chunk6(p, p + 1024, reinterpret_cast<char*>(p + 512), reinterpret_cast<char*>(p + 1536), 2048.0f,
                            [&](int k, int j) { return w[((long)(nt * 32 + j) * Cin + kc * 32 + k) * taps + tap]; });
            }
    return CER_OK;
}

// ------------------------------------------------------------------------------------------------------------- s16 stem (enc_stem.hip)

extern "C" long cer_enc_stem_s16_packed_size(void) { return 2L * SM_STEPS * 2 * 64 * 8; }     // halves: two layouts (below)

// w_oihw [32][3][7][7] (host) -> A fragments [step][hi | lo][lane][8]: lane (channel = lane & 31, kg = lane >> 5), element e:
// ky = step >> 1, column = 4 (step & 1) + 2 kg + (e >> 2), input channel = e & 3 (column 7 and channel 3 are padding: zero).
// A second copy follows with the padding column in FRONT (kernel column = that index - 1): the layout of enc_stem_pc_kernel, whose
// patch starts one image column earlier (16-byte aligned loads).  *log2s_w = the power-of-two weight scale that was applied.  The one pack
// that does not clamp.
extern "C" int cer_enc_stem_s16_pack(const float* w_oihw, void* packed_v, int* log2s_w) {
    if (!w_oihw || !packed_v || !log2s_w) return CER_EINVAL;
    double wmax = 0.0;
    for (int i = 0; i < 32 * 147; ++i) wmax = fmax(wmax, fabs((double)w_oihw[i]));
    int k = wmax > 0.0 ? (int)floor(log2(16384.0 / wmax)) : 0;
    if (k > 24) k = 24;
    if (k < -24) k = -24;
    *log2s_w = k;
    const float sc = ldexpf(1.0f, k);
    for (int layout = 0; layout < 2; ++layout)
        for (int s = 0; s < SM_STEPS; ++s)
            pack_slice((_Float16*)packed_v + (long)(layout * SM_STEPS + s) * 1024, 1.0f, [&](int k8, int ch) {
                const int ky = s >> 1, col = 4 * (s & 1) + 2 * (k8 >> 3) + ((k8 & 7) >> 2) - layout, ci = k8 & 3;
                return (col >= 0 && col < 7 && ci < 3) ? w_oihw[((ch * 3 + ci) * 7 + ky) * 7 + col] * sc : 0.f;
            }, false);
    return CER_OK;
}
