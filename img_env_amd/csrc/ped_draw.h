// ped_draw.h -- a robot's pedestrian map drawn again from its pedestrian vector.  k_obs (kernels.h) stamps the map from exactly the
// float32 (px, py, vx, vy) it has just stored as the first four of every pedestrian's seven floats, in rank order, with the handle's
// constants: the map is a pure function of the stored vector row, bit for bit.  So a rollout ring keeps the row (284 bytes at
// max_ped 10) and not the map (27 648 bytes at 48 x 48), and the map is drawn where it is read: into a minibatch, or for a caller.
//
// The definition (include/imgenv.h states it too).  v: a row of PV float32.  The output: [3][Hp][Wp] float32, every cell written.
//   n = v[0] truncated, clamped to [0, (PV - 1) / 7]; not finite or negative: 0
//   for q = 0 .. n - 1, ascending: (px, py, vx, vy) = v[1 + 7 q .. 4 + 7 q]
//     skipped where (double)px > 3 || < -3, the same for py (yaml_env.py:409), or where px / py is not a number
//     tmx = -(double)px + 3, tmy = -(double)py + 3
//     jj over [floor((tmx - r) / res), floor((tmx + r) / res)), kk likewise with tmy -- floor(x * ped_inv_res) where ped_inv_res != 0,
//       Python's x // ped_res otherwise (k_obs's two forms)
//     cell (jj, kk) inside [0, Hp) x [0, Wp) takes the disc where ((jj + 0.5) res - tmx)^2 + ((kk + 0.5) res - tmy)^2 < r^2, float64
//       in this order (the build has -ffp-contract=off)
//   a cell ends with the disc of the HIGHEST q that covers it: (1.0f, vx, vy), vx and vy copied bit for bit; none: (0, 0, 0)
//   a source row index below 0: an all-zero map
//
// k_ped_draw: a workgroup per output row, grid-strided over the rows.  "The highest q wins" needs no order between the discs:
//   (A) the rank plane -- Hp x Wp words of LDS -- is cleared; a lane per pedestrian puts q + 1 on its disc's cells with an LDS
//       atomicMax (more pedestrians than lanes: further rounds); a barrier
//   (B) the lanes walk the cells four at a time: one 16-byte LDS read of four ranks, vx and vy of the ranked pedestrians from the
//       row (a few cached words), one 16-byte store per plane: a wavefront writes 1 KB of consecutive bytes per plane and round
// A row without a source or without pedestrians skips (A).  No global atomics, no scratch.  The kernel is bound by its stores:
// 12 Hp Wp bytes written per row against 4 PV read.  Where Hp Wp is no multiple of 4 or the output is not 16-byte aligned, (B)
// stores word by word.
// The source row of output row i: i itself, rows[i], or the minibatch's order[first + i] (-1 from TR on; minibatch.h).
//
// ped_draw_src, ped_draw_count, ped_draw_stamp and ped_draw_store4 / _store1 are host / device functions:
// tests/host/ped_draw_check.cpp runs them over a simulated grid against tests/ped_draw_model.py.
#pragma once
#include <math.h>
#include <stdint.h>

#include "field_rows.h"   // FieldChunk16
#include "launch_plan.h"  // PED_DRAW_BLOCK, PED_DRAW_MAX_BLOCKS, PED_DRAW_LDS_BYTES
#include "tail_rows.h"    // TAIL_HD

#define PED_DRAW_ONE 0x3f800000u  // the bits of 1.0f

struct PedDrawDev {
    const float* vec;      // [.][PV]: the source rows
    float* out;            // [n][3][Hp][Wp]
    const int32_t* rows;   // [n] source row per output row, or nullptr ...
    const int32_t* order;  // ... or the minibatch's order [TR], read at first + i; both nullptr: row i
    size_t first;
    uint32_t TR;
    uint32_t n;            // output rows
    int32_t PV, Hp, Wp;
    int32_t wide;          // Hp Wp is a multiple of 4 and `out` 16-byte aligned: 16-byte stores
    double res, inv_res, r, r2;  // the handle's ped_res, ped_inv_res, ped_image_r, ped_image_r2
};

// Python float floor division (CPython float_floor_div), as k_obs's py_floordiv
TAIL_HD double ped_draw_floordiv(double vx, double wx) {
    double mod = fmod(vx, wx);
    double div = (vx - mod) / wx;
    if (mod != 0.0) {
        if ((wx < 0) != (mod < 0)) {
            mod += wx;
            div -= 1.0;
        }
    }
    double floordiv;
    if (div != 0.0) {
        floordiv = floor(div);
        if (div - floordiv > 0.5) floordiv += 1.0;
    } else {
        floordiv = copysign(0.0, vx / wx);
    }
    return floordiv;
}

// the source row of output row i, below 0 for none
TAIL_HD int64_t ped_draw_src(const PedDrawDev& d, size_t i) {
    if (d.order) {
        const size_t pos = d.first + i;
        return pos < (size_t)d.TR ? (int64_t)d.order[pos] : -1;
    }
    return d.rows ? (int64_t)d.rows[i] : (int64_t)i;
}

// the pedestrians of row v: v[0] truncated and clamped (a NaN fails the comparisons, an infinity the second; the cap is far below 2^24)
TAIL_HD int ped_draw_count(const float* v, int PV) {
    const float c = v[0];
    const int cap = (PV - 1) / 7;
    if (!(c >= 1.0f && c <= 3.402823466e38f)) return 0;
    return c >= (float)cap ? cap : (int)c;
}

// one bound of a disc's box, clipped to [0, cells] before it becomes an integer (cells outside the map take nothing anyway)
TAIL_HD int ped_draw_bound(const PedDrawDev& d, double x, int cells) {
    const double f = d.inv_res != 0.0 ? floor(x * d.inv_res) : ped_draw_floordiv(x, d.res);
    return f >= (double)cells ? cells : f > 0.0 ? (int)f : 0;
}

// pedestrian q of row v: put(cell, q + 1) for every cell of the map its disc covers
template <typename Put>
TAIL_HD void ped_draw_stamp(const PedDrawDev& d, const float* v, int q, Put&& put) {
    const float* o = v + 1 + 7 * (size_t)q;
    const double dpx = o[0], dpy = o[1];
    if (dpx > 3 || dpx < -3 || dpy > 3 || dpy < -3) return;  // yaml_env.py:409-410
    if (dpx != dpx || dpy != dpy) return;                    // (not a number: k_obs never stores one)
    const double tmx = -dpx + 3, tmy = -dpy + 3;
    const int ax = ped_draw_bound(d, tmx - d.r, d.Hp), bx = ped_draw_bound(d, tmx + d.r, d.Hp);
    const int ay = ped_draw_bound(d, tmy - d.r, d.Wp), by = ped_draw_bound(d, tmy + d.r, d.Wp);
    for (int jj = ax; jj < bx; jj++)
        for (int kk = ay; kk < by; kk++) {
            const double ddx = (jj + 0.5) * d.res - tmx, ddy = (kk + 0.5) * d.res - tmy;
            if (ddx * ddx + ddy * ddy < d.r2) put(jj * d.Wp + kk, (uint32_t)(q + 1));
        }
}

// the three words of a cell of rank `rank` (0: under no disc); vx and vy as the words they are
TAIL_HD void ped_draw_cell(const uint32_t* v, uint32_t rank, uint32_t& one, uint32_t& vx, uint32_t& vy) {
    one = vx = vy = 0u;
    if (rank) {
        const uint32_t* o = v + 1 + 7 * (size_t)(rank - 1);
        one = PED_DRAW_ONE;
        vx = o[2];
        vy = o[3];
    }
}
// cells 4 c .. 4 c + 3 of output row `o` ([3][NP] words) from their four ranks: one 16-byte store per plane
TAIL_HD void ped_draw_store4(const uint32_t* v, const FieldChunk16& ranks, uint32_t* o, size_t NP, size_t c) {
#if defined(__HIPCC__)
    const uint32_t r[4] = {ranks.x, ranks.y, ranks.z, ranks.w};
#else
    const uint32_t r[4] = {ranks.v[0], ranks.v[1], ranks.v[2], ranks.v[3]};
#endif
    uint32_t one[4], vx[4], vy[4];
    for (int k = 0; k < 4; k++) ped_draw_cell(v, r[k], one[k], vx[k], vy[k]);
#if defined(__HIPCC__)
    ((FieldChunk16*)o)[c] = make_uint4(one[0], one[1], one[2], one[3]);
    ((FieldChunk16*)(o + NP))[c] = make_uint4(vx[0], vx[1], vx[2], vx[3]);
    ((FieldChunk16*)(o + 2 * NP))[c] = make_uint4(vy[0], vy[1], vy[2], vy[3]);
#else
    for (int k = 0; k < 4; k++) {
        o[4 * c + k] = one[k];
        o[NP + 4 * c + k] = vx[k];
        o[2 * NP + 4 * c + k] = vy[k];
    }
#endif
}
// cell c alone, word by word
TAIL_HD void ped_draw_store1(const uint32_t* v, uint32_t rank, uint32_t* o, size_t NP, size_t c) {
    uint32_t one, vx, vy;
    ped_draw_cell(v, rank, one, vx, vy);
    o[c] = one;
    o[NP + c] = vx;
    o[2 * NP + c] = vy;
}

#if defined(__HIPCC__)
__global__ __launch_bounds__(PED_DRAW_BLOCK) void k_ped_draw(const PedDrawDev d) {
    extern __shared__ __attribute__((aligned(16))) uint32_t ped_draw_rank[];  // [Hp Wp]
    const size_t NP = (size_t)d.Hp * (size_t)d.Wp;
    const uint32_t tid = threadIdx.x;
    for (size_t i = blockIdx.x; i < (size_t)d.n; i += gridDim.x) {
        // (everything that decides a barrier is the same in every lane of the workgroup)
        const int64_t src = ped_draw_src(d, i);
        const float* v = d.vec + (size_t)(src < 0 ? 0 : src) * (size_t)d.PV;
        const int n = src < 0 ? 0 : ped_draw_count(v, d.PV);
        uint32_t* o = (uint32_t*)d.out + i * 3 * NP;
        if (n > 0) {
            for (size_t c = tid; c < NP; c += PED_DRAW_BLOCK) ped_draw_rank[c] = 0u;
            __syncthreads();
            for (int q = (int)tid; q < n; q += PED_DRAW_BLOCK)
                ped_draw_stamp(d, v, q, [&](int c, uint32_t rank) { atomicMax(&ped_draw_rank[c], rank); });
            __syncthreads();
        }
        if (d.wide) {
            for (size_t c = tid; c < NP / 4; c += PED_DRAW_BLOCK)
                ped_draw_store4((const uint32_t*)v, n > 0 ? ((const FieldChunk16*)ped_draw_rank)[c] : make_uint4(0u, 0u, 0u, 0u), o, NP, c);
        } else {
            for (size_t c = tid; c < NP; c += PED_DRAW_BLOCK) ped_draw_store1((const uint32_t*)v, n > 0 ? ped_draw_rank[c] : 0u, o, NP, c);
        }
        if (n > 0) __syncthreads();  // (the next row clears the plane)
    }
}
#endif
