// row_rebuild.h -- "write every output array of a resized Gaussian set in one launch", stated once for densify_apply_kernel
// (densify.hip) and mcmc_add_new_kernel (mcmc.hip).
//
// The grid is cut into segments, one per (group, array) and one per statistics array; a workgroup finds its segment from its block
// number and writes ROWSEG_CHUNK consecutive OUTPUT elements of it: coalesced float4 stores, gathered reads.  What an output row is
// made from (its entry) and what an element is worth belong to the operator; its kernel is
//
//   RowSeg G;
//   rowseg_find(G, a.seg, blockIdx.x);
//   rowseg_walk(G, a.P_new, [&](size_t row) { return <entry of row>; }, [&](Entry e, u32 c) { return <element c of that row>; });
//
// the one form whose generated code is not worse than the hand-written kernels' (profiles/row_rebuild/NOTES.md): a walker that is
// handed the kernel's parameter block, or a lookup that returns the segment, leaves the table in scratch.  Each translation unit
// keeps its own -ffp-contract=off: only the walk is here, no arithmetic on values.
#pragma once
#include "bags_common.h"

#define ROWSEG_BLOCK 256
#define ROWSEG_UNROLL 4
#define ROWSEG_CHUNK (ROWSEG_BLOCK * ROWSEG_UNROLL * 4)    // output elements per workgroup
#define ROWSEG_MAX_SEGS (3 * BAGS_DENSIFY_MAX_GROUPS + 3)  // parameter and two moments per group, three statistics arrays

// 1 and 2 are the operator's (densify: XYZ, SCALING; mcmc: OPACITY, SCALING)
enum { ROWSEG_COPY = 0, ROWSEG_MOMENT = 3, ROWSEG_ZERO = 4 };

struct RowSeg {
    const float* src; float* dst;
    u32 first_block;               // of this segment in the grid; 0xFFFFFFFF for an unused slot
    u32 width, mode, pad;
};

// Host: the segment table of one launch, for BagsDensifyGroup and BagsMcmcGroup alike: per group the parameter (mode_of(role)) and,
// with state, the two moments; then the three statistics arrays; unused slots never match a block.  Returns the grid size, or 0 where
// it would not fit the grid's 31 bits.
template <class Group, class ModeOf>
static inline unsigned rowseg_table(RowSeg (&seg)[ROWSEG_MAX_SEGS], const Group* groups, int n_groups, long long P_new, ModeOf mode_of,
                                    float* accum_out, float* denom_out, float* radii_out)
{
    size_t blocks = 0;
    int n_seg = 0;
    auto add = [&](const float* src, float* dst, int width, u32 mode) {
        seg[n_seg++] = RowSeg{src, dst, (u32)blocks, (u32)width, mode, 0};
        blocks += ((size_t)P_new * (size_t)width + ROWSEG_CHUNK - 1) / ROWSEG_CHUNK;
    };
    for (int k = 0; k < n_groups; ++k) {
        const Group& g = groups[k];
        add(g.param, g.param_out, g.width, mode_of(g.role));
        if (g.exp_avg) { add(g.exp_avg, g.exp_avg_out, g.width, ROWSEG_MOMENT); add(g.exp_avg_sq, g.exp_avg_sq_out, g.width, ROWSEG_MOMENT); }
    }
    add(nullptr, accum_out, 1, ROWSEG_ZERO); add(nullptr, denom_out, 1, ROWSEG_ZERO); add(nullptr, radii_out, 1, ROWSEG_ZERO);
    for (int k = n_seg; k < ROWSEG_MAX_SEGS; ++k) seg[k] = RowSeg{nullptr, nullptr, 0xFFFFFFFFu, 1, ROWSEG_ZERO, 0};
    return blocks >= 0x7FFFFFFFull ? 0u : (unsigned)blocks;
}

// the segment of block b: the last one of the table that starts at or before it
__device__ __forceinline__ void rowseg_find(RowSeg& G, const RowSeg* seg, const u32 b)
{
    G = seg[0];
#pragma unroll
    for (int k = 1; k < ROWSEG_MAX_SEGS; ++k)
        if (b >= seg[k].first_block) G = seg[k];
}

// The rest of a rebuild kernel, launched with ROWSEG_BLOCK threads on the grid rowseg_table returned.  G: this block's segment;
// row_of(row): the entry of an output row, read once per row; value_of(entry, c): element c of that row.
template <class Row, class Value>
__device__ __forceinline__ void rowseg_walk(const RowSeg& G, const long long P_new, const Row row_of, const Value value_of)
{
    const u32 b = blockIdx.x;
    const u32 w = G.width;
    const size_t n = (size_t)P_new * w;
    const size_t e0 = (size_t)(b - G.first_block) * ROWSEG_CHUNK;         // first element of the chunk, < n
    const size_t n4 = n >> 2;                                            // dst is 16-byte aligned (validated by the caller)
    float4* __restrict__ dst4 = reinterpret_cast<float4*>(G.dst);

    if (G.mode == ROWSEG_ZERO) {
#pragma unroll
        for (int j = 0; j < ROWSEG_UNROLL; ++j) {
            const size_t i = (e0 >> 2) + (size_t)j * ROWSEG_BLOCK + threadIdx.x;
            if (i < n4) dst4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if (e0 + ROWSEG_CHUNK >= n) { const size_t t = (n4 << 2) + threadIdx.x; if (t < n) G.dst[t] = 0.0f; }
        return;
    }

    const size_t row_base = e0 / w;                                      // wave-uniform
    const u32 rem_base = (u32)(e0 - row_base * w);                       // < w
#pragma unroll
    for (int j = 0; j < ROWSEG_UNROLL; ++j) {
        const u32 li = (u32)j * ROWSEG_BLOCK + threadIdx.x;              // float4 within the chunk
        const size_t i = (e0 >> 2) + li;
        if (i >= n4) continue;
        const u32 t = rem_base + 4u * li;                                // < w + ROWSEG_CHUNK
        const u32 q = t / w;
        u32 c = t - q * w;
        size_t row = row_base + q;
        auto ent = row_of(row);
        float o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {                                    // a float4 may cross a row boundary
            o[k] = value_of(ent, c);
            if (++c == w) { c = 0; ++row; if (k < 3 && row < (size_t)P_new) ent = row_of(row); }
        }
        dst4[i] = make_float4(o[0], o[1], o[2], o[3]);
    }
    if (e0 + ROWSEG_CHUNK >= n) {                                        // the n % 4 elements after the last float4
        const size_t t = (n4 << 2) + threadIdx.x;
        if (t < n) { const size_t row = t / w; G.dst[t] = value_of(row_of(row), (u32)(t - row * w)); }
    }
}
