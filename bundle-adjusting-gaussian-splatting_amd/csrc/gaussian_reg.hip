// gaussian_reg.hip -- the regularisers on the Gaussians themselves, over all P rows of the raw leaves _opacity (P,1) and _scaling
// (P,3), with Mip-Splatting's 3D filter f (P) where one is set and a row mask `select` (P bytes, NULL: every row):
//     unfiltered:  o = 1 / (1 + exp(-x)),  s_a = exp(r_a)
//     filtered:    e_a = exp(r_a),  s_a = sqrt(e_a^2 + f^2),  c = prod_a e_a / s_a,  o = sigmoid * c          (activations.hip's lines)
//     n = the number of selected rows;  kmin / kmax = the FIRST minimum / maximum of the row's raw r (s is monotone in r)
//     0 opacity  sum o / n                                   1 scale   sum sum_a s_a / (3 n)
//     2 flat     sum s_kmin / n                              3 aniso   sum max(s_kmax / s_kmin - max_ratio, 0) / n
//     4 big      sum sum_a max(s_a - max_scale, 0) / (3 n)   5 entropy sum -(o log o + (1 - o) log(1 - o)) / n
// Both hinges are strict (at the threshold: value and gradient zero); a row with o <= 0 or o >= 1 in float32 has no entropy and gets
// no gradient from it.  A term whose bit is not set in `terms` is an exact 0, sends no gradient, and its exp / sqrt / log are not
// evaluated.  n == 0: all six terms 0, all gradients 0.
//
// gr_row() forms a row's activations and takes its decisions in float32; the forward and the backward both call it, and the file is
// compiled with -ffp-contract=off, so the backward takes the decisions its forward took.  What is not a decision is formed so that
// it keeps its relative accuracy at the ends of the logit range: 1 - sigmoid as e sigmoid (e = exp(-x), x > 0, sigmoid < 1), 1 - c from
// 1 - e_a / s_a = f^2 / (s_a (s_a + e_a)), and log((1 - o) / o) of an unfiltered row as -x.  Sums and the gradient's combination are
// in double, each gradient rounded once.
//
// Forward: workgroup b takes the GR_ROWS rows from b * GR_ROWS on, thread t the rows t, t + 256, ... of them; a lane adds its rows
// in double, the workgroup adds its lanes (ordered_sum.h) and leaves one record of 8 doubles (six sums, the count, and a 0 it
// writes).  The finish kernel adds the records in index order (ordered_sum.h) and writes terms (6), count and the stats record
// (the six raw sums, n, 0).  No atomics, no memset.  Backward: a thread per row, every element of both outputs written
// (an unselected row: zeros); either output may be NULL.  The (P,3) rows are read and written as activations.hip does, element by
// element: no access is wider than 4 bytes, so any 4-byte-aligned tensor takes the one path there is.
#include "ordered_sum.h"

#define GR_BLOCK BAGS_GAUSSIAN_REG_BLOCK
#define GR_ROWS BAGS_GAUSSIAN_REG_ROWS
#define GR_REC BAGS_GAUSSIAN_REG_STATS               // doubles per workspace record and in the stats record
enum { GR_OPACITY = 1, GR_SCALE = 2, GR_FLAT = 4, GR_ANISO = 8, GR_BIG = 16, GR_ENTROPY = 32 };
enum { GR_N = 6 };                                   // index of the count in a record

struct GrDev {
    int P;
    unsigned terms;
    float max_ratio, max_scale;
    const float* opacity;
    const float* scaling;
    const float* filter;
    const unsigned char* select;
};

// what the wanted terms need of a row: the opacity chain, the scales (a filtered opacity needs them for c)
__device__ __forceinline__ bool gr_wants_o(const unsigned terms) { return (terms & (GR_OPACITY | GR_ENTROPY)) != 0; }
template <bool FILTER> __device__ __forceinline__ bool gr_wants_s(const unsigned terms)
{
    return (terms & (GR_SCALE | GR_FLAT | GR_ANISO | GR_BIG)) != 0 || (FILTER && gr_wants_o(terms));
}

struct GrRow {
    float x, sig, om;            // the logit, sigmoid, 1 - sigmoid
    float f2, e[3], s[3];        // f^2, exp(r_a), the activated scales (unfiltered: s = e)
    float c, omc;                // c and 1 - c (unfiltered: 1 and 0)
    float o, q;                  // the activated opacity and 1 - o
    float ratio;                 // s_kmax / s_kmin
    int kmin, kmax;
    bool aniso, big[3], entropy; // the decisions: ratio - max_ratio > 0, s_a - max_scale > 0, 0 < o < 1
};

template <bool FILTER> __device__ __forceinline__ void gr_row(const GrDev& a, const size_t i, GrRow& w)
{
    const unsigned t = a.terms;
    w.c = 1.0f; w.omc = 0.0f; w.f2 = 0.0f; w.ratio = 1.0f; w.kmin = 0; w.kmax = 0;
    w.aniso = false; w.entropy = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) { w.e[k] = 0.0f; w.s[k] = 0.0f; w.big[k] = false; }
    if (gr_wants_s<FILTER>(t)) {                                                             // uniform
        const float r0 = a.scaling[3 * i], r1 = a.scaling[3 * i + 1], r2 = a.scaling[3 * i + 2];
        w.kmin = (r1 < r0) ? 1 : 0;
        if (r2 < (w.kmin ? r1 : r0)) w.kmin = 2;
        w.kmax = (r1 > r0) ? 1 : 0;
        if (r2 > (w.kmax ? r1 : r0)) w.kmax = 2;
        w.e[0] = expf(r0); w.e[1] = expf(r1); w.e[2] = expf(r2);
        if (FILTER) {
            const float f = a.filter[i];
            w.f2 = f * f;
            float keep = 1.0f;                                                               // prod (1 - d_a), d_a = 1 - e_a / s_a
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                w.s[k] = sqrtf(w.e[k] * w.e[k] + w.f2);
                w.c *= w.e[k] / w.s[k];
                const float d = w.f2 / (w.s[k] * (w.s[k] + w.e[k]));
                w.omc = w.omc + keep * d;                                                    // 1 - c = d0 + (1-d0) d1 + (1-d0)(1-d1) d2
                keep *= 1.0f - d;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) w.s[k] = w.e[k];
        }
        if (t & GR_ANISO) {
            const float smax = w.kmax == 0 ? w.s[0] : (w.kmax == 1 ? w.s[1] : w.s[2]);
            const float smin = w.kmin == 0 ? w.s[0] : (w.kmin == 1 ? w.s[1] : w.s[2]);
            w.ratio = smax / smin;
            w.aniso = w.ratio - a.max_ratio > 0.0f;
        }
        if (t & GR_BIG) {
#pragma unroll
            for (int k = 0; k < 3; ++k) w.big[k] = w.s[k] - a.max_scale > 0.0f;
        }
    }
    w.x = 0.0f; w.sig = 0.0f; w.om = 1.0f; w.o = 0.0f; w.q = 1.0f;
    if (gr_wants_o(t)) {                                                                     // uniform
        w.x = a.opacity[i];
        const float en = expf(-w.x);
        w.sig = 1.0f / (1.0f + en);
        // 1 - sigmoid without the cancellation at large logits; a sigmoid that is 1 in float32 has no slope (as in activations.hip)
        w.om = w.x > 0.0f ? (w.sig < 1.0f ? en * w.sig : 0.0f) : 1.0f - w.sig;
        w.o = FILTER ? w.sig * w.c : w.sig;
        w.q = FILTER ? w.om + w.sig * w.omc : w.om;
        // (q > 0 follows from o < 1; it is asked so that no log(0) can reach a sum whatever the inputs are)
        w.entropy = (t & GR_ENTROPY) && w.o > 0.0f && w.o < 1.0f && w.q > 0.0f;
    }
}

__device__ __forceinline__ bool gr_selected(const GrDev& a, const size_t i) { return !a.select || a.select[i] != 0; }

template <bool FILTER>
__global__ void __launch_bounds__(GR_BLOCK) gaussian_reg_sums_kernel(const GrDev a, double* __restrict__ records)
{
    __shared__ double sh[GR_BLOCK / 64 * GR_REC];
    double acc[GR_N + 1];
#pragma unroll
    for (int t = 0; t <= GR_N; ++t) acc[t] = 0.0;
    const size_t first = (size_t)blockIdx.x * GR_ROWS + threadIdx.x;
#pragma unroll
    for (int j = 0; j < GR_ROWS / GR_BLOCK; ++j) {
        const size_t i = first + (size_t)j * GR_BLOCK;
        if (i >= (size_t)a.P || !gr_selected(a, i)) continue;
        GrRow w;
        gr_row<FILTER>(a, i, w);
        acc[GR_N] += 1.0;
        if (a.terms & GR_OPACITY) acc[0] += (double)w.o;
        if (a.terms & GR_SCALE) acc[1] += ((double)w.s[0] + (double)w.s[1]) + (double)w.s[2];
        if (a.terms & GR_FLAT) acc[2] += (double)(w.kmin == 0 ? w.s[0] : (w.kmin == 1 ? w.s[1] : w.s[2]));
        if (w.aniso) acc[3] += (double)(w.ratio - a.max_ratio);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (w.big[k]) acc[4] += (double)(w.s[k] - a.max_scale);
        if (w.entropy) acc[5] -= (double)w.o * (double)logf(w.o) + (double)w.q * (double)logf(w.q);
    }
    osum::block_sum<GR_N + 1>(acc, sh);                                                      // every lane is here
    if (threadIdx.x < GR_REC)
        records[(size_t)blockIdx.x * GR_REC + threadIdx.x] = ((int)threadIdx.x <= GR_N) ? osum::block_total<GR_N + 1>(sh, threadIdx.x) : 0.0;
}

// One workgroup: the nrec records added in index order (ordered_sum.h), then the six terms, the count and the stats record.
// nrec == 0 (P == 0): zeros.
__global__ void __launch_bounds__(256) gaussian_reg_finish_kernel(const int nrec, const double* __restrict__ records, float* __restrict__ terms,
                                                                  float* __restrict__ count, double* __restrict__ stats)
{
    __shared__ double sh[4 * (GR_N + 1)];
    double S[GR_N + 1];
    osum::ordered_rows_sum<GR_N + 1>(records, nrec, GR_REC, sh, S);
    if (threadIdx.x != 0) return;
    const double n = S[GR_N];
    const double inv_n = n > 0.0 ? 1.0 / n : 0.0, inv_3n = n > 0.0 ? 1.0 / (3.0 * n) : 0.0;
    terms[0] = (float)(S[0] * inv_n);
    terms[1] = (float)(S[1] * inv_3n);
    terms[2] = (float)(S[2] * inv_n);
    terms[3] = (float)(S[3] * inv_n);
    terms[4] = (float)(S[4] * inv_3n);
    terms[5] = (float)(S[5] * inv_n);
    count[0] = (float)n;
#pragma unroll
    for (int c = 0; c <= GR_N; ++c) stats[c] = S[c];
    stats[GR_N + 1] = 0.0;
}

// dL/d_opacity (P) and dL/d_scaling (P,3) of L = sum_k g_k terms_k, every element (an unselected row, n == 0: zeros); either may be
// NULL, and what is stored is the same bits whichever is wanted.  With G_o and G_a the cotangents of o and of s_a:
//     G_o = g0 / n + (g5 / n) log((1 - o) / o)                                                          [entropy: where 0 < o < 1]
//     G_a = g1 / 3n + [a = kmin] g2 / n + [ratio > max_ratio] (g3 / n) ([a = kmax] / s_kmin - [a = kmin] s_kmax / s_kmin^2)
//           + [s_a > max_scale] g4 / 3n
//     dL/dx = G_o c sigmoid (1 - sigmoid) ;  dL/dr_a = G_a ds_a/dr_a + G_o sigmoid c f^2 / s_a^2        (activations.hip: through_c)
//     ds_a/dr_a = s_a (unfiltered), e_a^2 / s_a (filtered)
template <bool FILTER>
__global__ void __launch_bounds__(GR_BLOCK) gaussian_reg_bwd_kernel(const GrDev a, const double* __restrict__ stats, const float* __restrict__ g_terms,
                                                                   float* __restrict__ g_opacity, float* __restrict__ g_scaling)
{
    const size_t i = (size_t)blockIdx.x * GR_BLOCK + threadIdx.x;
    if (i >= (size_t)a.P) return;
    const double n = stats[GR_N];
    double go = 0.0, gr[3] = {0.0, 0.0, 0.0};
    if (n > 0.0 && gr_selected(a, i)) {
        const double inv_n = 1.0 / n, inv_3n = 1.0 / (3.0 * n);
        const unsigned t = a.terms;
        const double w0 = (t & GR_OPACITY) ? (double)g_terms[0] * inv_n : 0.0, w1 = (t & GR_SCALE) ? (double)g_terms[1] * inv_3n : 0.0;
        const double w2 = (t & GR_FLAT) ? (double)g_terms[2] * inv_n : 0.0, w3 = (t & GR_ANISO) ? (double)g_terms[3] * inv_n : 0.0;
        const double w4 = (t & GR_BIG) ? (double)g_terms[4] * inv_3n : 0.0, w5 = (t & GR_ENTROPY) ? (double)g_terms[5] * inv_n : 0.0;
        GrRow w;
        gr_row<FILTER>(a, i, w);
        double Go = w0;
        if (w.entropy) Go += w5 * (FILTER ? (double)logf(w.q) - (double)logf(w.o) : -(double)w.x);
        if (gr_wants_o(t)) go = ((Go * (double)w.c) * (double)w.sig) * (double)w.om;
        if (gr_wants_s<FILTER>(t)) {
            const double smin = (double)(w.kmin == 0 ? w.s[0] : (w.kmin == 1 ? w.s[1] : w.s[2]));
            const double smax = (double)(w.kmax == 0 ? w.s[0] : (w.kmax == 1 ? w.s[1] : w.s[2]));
            const double through_c = FILTER ? ((Go * (double)w.sig) * (double)w.c) * (double)w.f2 : 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                double Ga = w1;
                if (k == w.kmin) Ga += w2;
                if (w.aniso) {
                    if (k == w.kmax) Ga += w3 / smin;
                    if (k == w.kmin) Ga -= (w3 * smax) / (smin * smin);
                }
                if (w.big[k]) Ga += w4;
                const double sk = (double)w.s[k], ek = (double)w.e[k];
                gr[k] = FILTER ? Ga * ((ek * ek) / sk) + through_c / (sk * sk) : Ga * sk;
            }
        }
    }
    if (g_opacity) g_opacity[i] = (float)go;                                                 // uniform
    if (g_scaling) {
        g_scaling[3 * i] = (float)gr[0]; g_scaling[3 * i + 1] = (float)gr[1]; g_scaling[3 * i + 2] = (float)gr[2];
    }
}

// workgroups (= records) of the sums kernel: a function of P alone
int gaussian_reg_records(int P) { return P > 0 ? (int)(((long long)P + GR_ROWS - 1) / GR_ROWS) : 0; }

static GrDev gr_dev(const BagsGaussianReg& a)
{
    GrDev d{};
    d.P = a.P; d.terms = a.terms; d.max_ratio = a.max_ratio; d.max_scale = a.max_scale;
    d.opacity = a.opacity_raw; d.scaling = a.scaling_raw; d.filter = a.filter;
    d.select = reinterpret_cast<const unsigned char*>(a.select);
    return d;
}

// the struct is validated by the caller (api.hip); records: gaussian_reg_records(P) records of 8 doubles (none for P == 0)
hipError_t launch_gaussian_reg_fwd(const BagsGaussianReg& a, double* records, float* terms, float* count, double* stats, hipStream_t st)
{
    const GrDev d = gr_dev(a);
    const int nrec = gaussian_reg_records(a.P);
    if (nrec > 0) {
        const hipError_t e = with_bool(a.filter != nullptr, [&](auto F) {
            hipLaunchKernelGGL((gaussian_reg_sums_kernel<decltype(F)::value>), dim3((unsigned)nrec), dim3(GR_BLOCK), 0, st, d, records);
            return hipGetLastError(); });
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(gaussian_reg_finish_kernel, dim3(1), dim3(256), 0, st, nrec, records, terms, count, stats);
    return hipGetLastError();
}

hipError_t launch_gaussian_reg_bwd(const BagsGaussianReg& a, const double* stats, const float* g_terms, float* g_opacity, float* g_scaling,
                                   hipStream_t st)
{
    if (a.P <= 0 || (!g_opacity && !g_scaling)) return hipSuccess;
    const GrDev d = gr_dev(a);
    const unsigned blocks = (unsigned)(((long long)a.P + GR_BLOCK - 1) / GR_BLOCK);
    return with_bool(a.filter != nullptr, [&](auto F) {
        hipLaunchKernelGGL((gaussian_reg_bwd_kernel<decltype(F)::value>), dim3(blocks), dim3(GR_BLOCK), 0, st, d, stats, g_terms, g_opacity,
                           g_scaling);
        return hipGetLastError(); });
}
