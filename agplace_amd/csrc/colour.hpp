// Colour jitter arithmetic of the camera front end: torchvision's ColorJitter on a PIL frame, i.e. Pillow's
// Image.blend against a degenerate image (ImageEnhance) and Pillow's RGB <-> HSV conversions (libImaging/Convert.c), operation
// for operation.  Host and device compile the same text (tools/colour_host_check.cpp runs it on the CPU), so nothing here may
// be contracted into a fused multiply-add: Pillow's C rounds every product and every sum on its own.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AGP_HD __host__ __device__ inline
#else
#define AGP_HD inline
#endif

#pragma clang fp contract(off)

namespace agp_colour {

enum { OP_NONE = 0, OP_BRIGHTNESS = 1, OP_CONTRAST = 2, OP_SATURATION = 3, OP_HUE = 4 };
constexpr int RECORD = 8;      // floats per frame: 4 ops in order, 3 factors (brightness, contrast, saturation), the hue byte shift

struct rgb8 { int r, g, b; };

// Pillow's convert("L")
AGP_HD int luma(rgb8 p) { return (19595 * p.r + 38470 * p.g + 7471 * p.b + 0x8000) >> 16; }

// Image.blend(degenerate, image, a) for one byte: t = fl32(deg + fl32(a * (x - deg))); x - deg is exact.  For 0 <= a <= 1 Pillow
// truncates t, which lies in [0, 255] there, so the clipping branch gives the same byte
AGP_HD int blend(int deg, int x, float a) {
    const float d = (float)deg;
    const float prod = a * (float)(x - deg);
    const float t = d + prod;
    if (!(t > 0.f)) return 0;      // (a NaN from a non-finite factor too: no undefined conversion)
    if (t >= 255.f) return 255;
    return (int)t;
}

AGP_HD int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// Pillow's rgb2hsv: (H, S, V) in .r, .g, .b
AGP_HD rgb8 rgb_to_hsv(rgb8 p) {
    const int maxc = p.r > p.g ? (p.r > p.b ? p.r : p.b) : (p.g > p.b ? p.g : p.b);
    const int minc = p.r < p.g ? (p.r < p.b ? p.r : p.b) : (p.g < p.b ? p.g : p.b);
    rgb8 o = {0, 0, maxc};
    if (maxc == minc) return o;
    const float cr = (float)(maxc - minc);
    const float s = cr / (float)maxc;
    const float rc = (float)(maxc - p.r) / cr, gc = (float)(maxc - p.g) / cr, bc = (float)(maxc - p.b) / cr;
    float h;
    if (p.r == maxc) h = (float)((double)bc - (double)gc);
    else if (p.g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
    else h = (float)(4.0 + (double)gc - (double)rc);
    h = (float)fmod((double)h / 6.0 + 1.0, 1.0);
    o.r = clip8((int)((double)h * 255.0));
    o.g = clip8((int)((double)s * 255.0));
    return o;
}

// Pillow's hsv2rgb: (H, S, V) in .r, .g, .b
AGP_HD rgb8 hsv_to_rgb(rgb8 p) {
    const int H = p.r, S = p.g, V = p.b;
    rgb8 o = {V, V, V};
    if (S == 0) return o;
    const double h6 = (double)(float)H * 6.0 / 255.0;
    const int i = (int)floor(h6);
    const double f = (double)(float)(h6 - (double)(float)i);
    const double fs = (double)(float)((double)(float)S / 255.0);
    const double v = (double)(float)V;
    const int pp = clip8((int)round(v * (1.0 - fs)));
    const int q = clip8((int)round(v * (1.0 - fs * f)));
    const int t = clip8((int)round(v * (1.0 - fs * (1.0 - f))));
    switch (i % 6) {
        case 0: o.r = V; o.g = t; o.b = pp; break;
        case 1: o.r = q; o.g = V; o.b = pp; break;
        case 2: o.r = pp; o.g = V; o.b = t; break;
        case 3: o.r = pp; o.g = q; o.b = V; break;
        case 4: o.r = t; o.g = pp; o.b = V; break;
        default: o.r = V; o.g = pp; o.b = q; break;
    }
    return o;
}

// One frame's record as the kernels hold it
struct record {
    int op[4];
    float fb, fc, fs;
    int shift;
};

// ops are small integers stored as floats; anything else (NaN included) reads as OP_NONE
AGP_HD record load_record(const float* r) {
    record c;
    for (int k = 0; k < 4; ++k) {
        const float v = r[k];
        c.op[k] = (v >= 1.f && v <= 4.f) ? (int)v : OP_NONE;
    }
    c.fb = r[4]; c.fc = r[5]; c.fs = r[6];
    const float sh = r[7];
    c.shift = (sh >= 0.f && sh <= 255.f) ? (int)sh : 0;
    return c;
}

AGP_HD int contrast_pos(const record& c) {
    for (int k = 0; k < 4; ++k)
        if (c.op[k] == OP_CONTRAST) return k;
    return -1;
}

// ImageEnhance.Contrast's grey level int(sum / count + 0.5) in integers (sum <= 255 * count, count < 2^31)
AGP_HD int contrast_mean(uint64_t sum, uint64_t count) { return (int)((2 * sum + count) / (2 * count)); }

// ops [k0, k1) of a record on one pixel; `m` is the contrast grey level (used only when contrast lies in the range)
AGP_HD rgb8 apply_ops(rgb8 p, const record& c, int k0, int k1, int m) {
    for (int k = k0; k < k1; ++k) {
        switch (c.op[k]) {
            case OP_BRIGHTNESS: p.r = blend(0, p.r, c.fb); p.g = blend(0, p.g, c.fb); p.b = blend(0, p.b, c.fb); break;
            case OP_CONTRAST: p.r = blend(m, p.r, c.fc); p.g = blend(m, p.g, c.fc); p.b = blend(m, p.b, c.fc); break;
            case OP_SATURATION: {
                const int l = luma(p);
                p.r = blend(l, p.r, c.fs); p.g = blend(l, p.g, c.fs); p.b = blend(l, p.b, c.fs);
                break;
            }
            case OP_HUE: {
                rgb8 q = rgb_to_hsv(p);
                q.r = (q.r + c.shift) & 255;
                p = hsv_to_rgb(q);
                break;
            }
            default: break;
        }
    }
    return p;
}

// torchvision's CenterCrop(c) origin along one axis: Python's round((n - c) / 2.0), halves to even
AGP_HD int crop_origin(int n, int c) {
    const int d = n - c, k = d >> 1;
    return (d & 1) ? k + (k & 1) : k;
}

}  // namespace agp_colour
