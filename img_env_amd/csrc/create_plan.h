// create_plan.h -- what imgenv_create decides before it touches a device: the refusals of its arguments, the grid the handle works
// on, the class layer's mode and the bit budget of its SUM word, the rasters' boxes, the sub-steps, the early-observation rule, the
// LDS sizes and the layout of the output arena.  Host code, nothing of HIP: plain C++17, compiled by g++ for
// tests/host/create_plan_check.cpp.  imgenv_hip.hip checks, plans, then allocates what the plan says (its create_* phases).
//
// A refusal returns its IMGENV_E* code and leaves its text in `msg`; the caller hands both on (imgenv_last_error).
#pragma once
#include <math.h>
#include <stdio.h>

#include <vector>

#include "host_tables.h"  // ViewGeom, RobotClassHost, PedClassHost
#include "launch_plan.h"
#include "out_fields.h"

typedef char CreateMsg[512];
#define REFUSE(code, ...) return snprintf(msg, sizeof(CreateMsg), __VA_ARGS__), (code)

inline int shard_of(const imgenv_cfg& c, int& r0, int& r1) {
    r0 = c.robot_begin;
    r1 = c.robot_end;
    if (r0 == 0 && r1 == 0) r1 = c.n_robots;
    if (r0 < 0 || r1 > c.n_robots || r0 >= r1) return -1;
    return 0;
}

// ---------------------------------------------------------------------------------------- the arguments
struct CreateArgs {  // what the argument checks settle on their way
    int W, r0, r1;
    bool beep_on, view_resize;
    ViewGeom g;
};
inline int create_check_args(const imgenv_cfg* cfg, bool has_map, bool has_out, int Hg, int Wg, CreateArgs& a, CreateMsg& msg) {
    if (!cfg || !has_map || !has_out) REFUSE(IMGENV_EINVAL, "null argument");
    if (cfg->abi_version != IMGENV_ABI_VERSION || cfg->struct_size != (int32_t)sizeof(imgenv_cfg))
        REFUSE(IMGENV_EINVAL, "imgenv_cfg ABI mismatch (version %d size %d, want %d %d)", cfg->abi_version,
               cfg->struct_size, IMGENV_ABI_VERSION, (int)sizeof(imgenv_cfg));
    if (cfg->n_robots < 1 || cfg->n_peds < 0 || Hg < 1 || Wg < 1) REFUSE(IMGENV_EINVAL, "bad sizes");
    const int W = a.W = cfg->n_worlds > 1 ? cfg->n_worlds : 1;
    if (cfg->n_robots % W || cfg->n_peds % W)
        REFUSE(IMGENV_EINVAL, "n_robots %d and n_peds %d must be multiples of n_worlds %d", cfg->n_robots, cfg->n_peds, W);
    if (cfg->n_peds / W > cfg->max_ped)
        REFUSE(IMGENV_EINVAL, "n_peds %d > max_ped %d (IndexError in yaml_env.py:401)", cfg->n_peds / W, cfg->max_ped);
    if (cfg->n_peds / W > 65000) REFUSE(IMGENV_EINVAL, "more than 65000 pedestrians in one world unsupported");
    if (cfg->n_robots >= (int)OWNER_MULTI) REFUSE(IMGENV_EINVAL, "more than 2^24 - 3 robots unsupported");
    if (cfg->image_size[0] < 1 || cfg->image_size[1] < 1) REFUSE(IMGENV_EINVAL, "bad image_size");
    if (cfg->state_dim < 3 || cfg->state_dim > 5) REFUSE(IMGENV_EINVAL, "state_dim must be 3, 4 or 5");
    if (cfg->ped_vec_dim != 7) REFUSE(IMGENV_EINVAL, "ped_vec_dim must be 7");
    if (cfg->ped_scene_type == IMGENV_SCENE_PEDSIM) {
        const int n_sfm = (cfg->n_peds + (cfg->relation_ped_robo == 1 ? cfg->n_robots : 0)) / W;  // one crowd (one PedScene) per world
        if (cfg->relation_ped_robo == 1 && cfg->n_robots / W > 8)
            REFUSE(IMGENV_EINVAL, "pedscene with relation_ped_robo=1 and more than 8 robots: the reference node recurses forever in "
                                  "Ttree::addAgent (all robot Tagents start at (0,0,0), ped_tree.cpp:65-96)");
        if (n_sfm > SFM_MAX_AGENTS) REFUSE(IMGENV_EINVAL, "pedscene crowds larger than %d agents are not supported", SFM_MAX_AGENTS);
    }
    if (shard_of(*cfg, a.r0, a.r1)) REFUSE(IMGENV_EINVAL, "bad robot shard [%d,%d)", cfg->robot_begin, cfg->robot_end);
    // The lottery only ever has an effect in the ERVO scene (rs_ / ps_ are ignored by the others, img_env.cpp:343).
    a.beep_on = cfg->ped_scene_type == IMGENV_SCENE_ERVO && cfg->n_peds > 0 && cfg->beep_r > 0 && cfg->ped_ca_p > 0;
    if (a.beep_on && a.r1 - a.r0 != cfg->n_robots)
        REFUSE(IMGENV_EINVAL, "beep_r / ped_ca_p > 0 in a robot shard: the beep lottery needs every robot's action on every rank");
    if (W > 1 && a.r1 - a.r0 != cfg->n_robots)
        REFUSE(IMGENV_EINVAL, "n_worlds > 1 cannot be combined with a robot shard: give each rank whole worlds (its own handle)");
    a.g = make_view_geom(*cfg);
    if (a.g.Hv < 1 || a.g.Wv < 1 || a.g.Hv > 4096 || a.g.Wv > 4096) REFUSE(IMGENV_EINVAL, "view of %d x %d cells unsupported", a.g.Hv, a.g.Wv);
    if (a.g.B > 65535) REFUSE(IMGENV_EINVAL, "more than 65535 beams unsupported");
    // cv2.resize(view, (image_size[0], image_size[1]), INTER_CUBIC) (yaml_env.py:431-438): dsize = (width, height)
    a.view_resize = cfg->image_size[0] != a.g.Wv || cfg->image_size[1] != a.g.Hv;
    return IMGENV_OK;
}

inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// The grid the handle works on.  GridMap::read_image (grid_map.cpp:28-38): where the resolutions differ the image is resized
// (INTER_LINEAR) to the view resolution; Hg x Wg come in as the map was given and leave as that grid.  The kernels index the worlds'
// copies of a layer with 32 bits: checked on the grid the handle really works on.
inline int create_grid_size(const imgenv_cfg& c, int W, int& Hg, int& Wg, CreateMsg& msg) {
    const bool resized = c.global_resolution != c.view_resolution;
    if (resized) {
        const double resolution_ = (double)c.global_resolution, view_res = (double)c.view_resolution;
        const double w2d = floor(Wg * resolution_ / view_res), h2d = floor(Hg * resolution_ / view_res);  // (range-checked before the cast)
        if (!(w2d >= 1 && h2d >= 1 && w2d * h2d < 2147483648.0)) REFUSE(IMGENV_EINVAL, "the map would be resized to %.0f x %.0f cells", h2d, w2d);
        Hg = (int)h2d;
        Wg = (int)w2d;
    }
    if (W > 1 && align16((size_t)Hg * Wg) * (size_t)W >= ((size_t)1 << 32)) {
        if (resized) REFUSE(IMGENV_EINVAL, "n_worlds x map cells must stay below 2^32 (the map is resized to %d x %d cells)", Hg, Wg);
        REFUSE(IMGENV_EINVAL, "n_worlds x map cells must stay below 2^32");
    }
    return IMGENV_OK;
}

inline int create_check_shapes(const imgenv_cfg& c, CreateMsg& msg) {
    for (int i = 0; i < c.n_robots; i++)
        if (c.robot_shape[i] != IMGENV_SHAPE_CIRCLE && c.robot_shape[i] != IMGENV_SHAPE_RECTANGLE)
            REFUSE(IMGENV_EINVAL, "robot %d: unsupported shape %d", i, c.robot_shape[i]);
    return IMGENV_OK;
}

// ---------------------------------------------------------------------------------------- the class layer
// How is the class layer kept up to date?  Composed: the rasters fill two owner layers and a pedestrian layer with
// fire-and-forget atomics and k_compose merges (and re-arms) them every step -- 14 bytes a cell, every cell of every
// world.  Stamped: the rasters merge their stamps straight onto the class layer (compare-and-swap) and stamps expire
// by their step tag -- nothing per cell, but slower rasters and a slightly longer decode in k_view.  Composed wins
// where the agents cover a good part of the map (the headline world: 0.133 against 0.138 ms per step), stamped
// where the maps are much larger than what the agents touch (8192 one-robot worlds: 52 against 43 M robot-steps/s).
// ... and where the owner layers + k_compose used to be the answer, the counting layer is (round 5: no pass over every cell
// of every world per step, a robot that covers the same cells as a step ago issues no atomic at all) -- wherever it can
// run: every footprint fits the rasters' LDS box, views through k_view, and the word has room for the counts: 3 bits of
// base class, as many pedestrian bits as a world has pedestrians, the robot's index within its world, and at least 6 bits
// of robot count.  A robot SHARD (round 6; world.h: sum_shard) numbers its own robots 1 .. RL in the index field and needs
// every footprint's box to fit a 64-bit bitmap, which is how the other ranks' robots arrive.
struct LayerPlan {
    bool stamp = false, sum = false, sum_shard = false;
    int pc_bits = 0, id_bits = 0;
    uint32_t sum_pc_mask = 0, sum_rc_shift = 0, sum_id_shift = 0;  // (0 unless sum)
    unsigned long long sum_wg_magic = 0;
    int rm_rad = 0;  // a shard in SUM mode: the radius of the other ranks' bitmaps where every class has the same, else -1
};
inline int bits_to_count(int v) {  // bits to count up to v
    int b = 0;
    while ((1 << b) <= v) b++;
    return b;
}
inline LayerPlan plan_layer_mode(int R, int RL, int P, int W, int Hg, int Wg, uint32_t flags, const std::vector<RobotClassHost>& rcls,
                                 const std::vector<PedClassHost>& pcls) {
    LayerPlan l;
    const size_t G = (size_t)Hg * Wg;
    l.stamp = plan_layer_stamp(RL == R, G * W, R, P, flags);  // (where each wins, measured: launch_plan.h)
    const bool shard = RL != R;
    l.id_bits = shard ? bits_to_count(RL) : std::max(1, bits_to_count(R / W - 1));
    l.pc_bits = bits_to_count(P / W);
    bool fits = G < ((size_t)1 << 24) && 3 + l.pc_bits + 6 + l.id_bits <= 32;
    for (const RobotClassHost& k : rcls)
        fits = fits && !k.big && (2 * k.box_rad + 1) * (2 * k.box_rad + 1) <= RASTER_BOX_CELLS &&
               (!shard || (2 * k.box_rad - 3) * (2 * k.box_rad - 3) <= WAVE);  // (the bitmap: the box without its margin of two cells)
    for (const PedClassHost& k : pcls) fits = fits && (2 * k.box_rad + 1) * (2 * k.box_rad + 1) <= RASTER_BOX_CELLS;
    const bool want_sum = (flags & IMGENV_FLAG_LAYER_SUM) != 0 || (!l.stamp && !(flags & IMGENV_FLAG_COMPOSE_DENSE));
    l.sum = want_sum && fits;
    if (l.sum) {
        l.stamp = false;
        l.sum_shard = shard;
        l.sum_pc_mask = (1u << l.pc_bits) - 1u;
        l.sum_rc_shift = 3u + (uint32_t)l.pc_bits;
        l.sum_id_shift = 32u - (uint32_t)l.id_bits;
        l.sum_wg_magic = (((unsigned long long)1 << 40) + (unsigned long long)Wg - 1) / (unsigned long long)Wg;
    }
    if (l.sum_shard) {
        l.rm_rad = rcls[0].box_rad - 2;
        for (const RobotClassHost& k : rcls)
            if (k.box_rad - 2 != l.rm_rad) l.rm_rad = -1;
    }
    return l;
}

// ---------------------------------------------------------------------------------------- smaller facts
// while (cur_control <= step_hz) { ...; cur_control += 0.05; } with the loop's own fp64 accumulation
inline int plan_n_sub(double step_hz) {
    double cur = 0;
    int n_sub = 0;
    while (cur <= step_hz && n_sub < (1 << 20)) {
        n_sub++;
        cur += 0.05;
    }
    return n_sub;
}
inline bool plan_pow2(double res) {  // exact power of two: x * (1/res) == x / res bit for bit
    int e = 0;
    return frexp(res, &e) == 0.5;
}
// early-observation steps: worlds owned whole, an ORCA crowd that nothing but the solve moves (no beep lottery), no
// limiter history to carry, views through k_view -- the headline shape and cfg-5; everything else keeps k_obs behind the move
// ... or a social-force crowd that is stepped a step ahead (sfm_ahead): its arrays are published in front of the move and
// stand still during the step, so the early k_obs reads them as they are (obs_early = 2); the gate also says that the
// publishing is done
// (robot shards too, since round 6: k_obs reads the rank's own robots' snapshots and the replicated pedestrians')
inline bool plan_early_obs(bool serial, int P, int NA, bool sfm_ahead, bool beep_on, bool limiters, bool big_view, int n_sub) {
    return !serial && P > 0 && (NA > 0 || sfm_ahead) && !beep_on && !limiters && !big_view && plan_integrate_fits(n_sub);
}
inline bool cfg_has_limiters(const imgenv_cfg& c) {
    return c.limiter_v.has_velocity_limits || c.limiter_v.has_acceleration_limits || c.limiter_v.has_jerk_limits ||
           c.limiter_w.has_velocity_limits || c.limiter_w.has_acceleration_limits || c.limiter_w.has_jerk_limits;
}

// ---------------------------------------------------------------------------------------- the plan
struct CreatePlan {
    int R, P, RL, r0, r1, W, Rw, Pw, NA, Hg, Wg;
    bool beep_on, view_resize, serial, full_rewrite;
    size_t G, Gs, Gp;  // cells of the grid, between two worlds' copies of a layer, of a layer of every world
    bool pow2;
    uint32_t wv_magic;
    double ped_res, ped_inv_res;
    int n_sub;
    LayerPlan layer;
    bool big_view;
    int box_cells, fp_cap, pd_cap, region_margin;  // k_raster's LDS box, the footprint and pedestrian cell lists (pd_cap: SUM only)
    int hit_stride;
    int big_words = 0, big_hit_stride = 0, big_full_chunks = 1;  // (big views only)
    bool big_bits_in_lds = true;
    int PP, obs_E, obs_passes;  // sort slots of k_obs, per lane (0: LDS sort), passes of its incremental sort (obs_E >= 2)
    size_t lds_view, lds_obs, lds_view_big = 0;
    bool sfm_ahead, early;
    OutFacts out;
    ArenaLayout arena;
};

// ... from the checked arguments, the grid and the class tables (create_classes).  The refusals that need the tables, in front of
// the first allocation.
inline int plan_create(const imgenv_cfg& c, const CreateArgs& a, int Hg, int Wg, bool serial, const std::vector<RobotClassHost>& rcls,
                       const std::vector<PedClassHost>& pcls, CreatePlan& p, CreateMsg& msg) {
    const ViewGeom& g = a.g;
    const int W = a.W;
    p.R = c.n_robots; p.P = c.n_peds; p.r0 = a.r0; p.r1 = a.r1; p.RL = a.r1 - a.r0;
    p.W = W; p.Rw = p.R / W; p.Pw = p.P / W; p.Hg = Hg; p.Wg = Wg;
    p.beep_on = a.beep_on; p.view_resize = a.view_resize; p.serial = serial;
    const bool rvo = (c.ped_scene_type == IMGENV_SCENE_RVO || c.ped_scene_type == IMGENV_SCENE_ERVO);
    p.NA = rvo ? p.P + (c.relation_ped_robo == 1 ? p.R : 0) : 0;
    p.G = (size_t)Hg * Wg;
    p.Gs = W > 1 ? align16(p.G) : p.G;
    p.Gp = W > 1 ? p.Gs * W : align16(p.G);
    p.pow2 = plan_pow2(g.res);
    p.wv_magic = (uint32_t)((0x100000000ull + (uint64_t)g.Wv - 1) / (uint64_t)g.Wv);
    p.ped_res = 6.0 / c.ped_image_size[0];  // yaml_env.py:164
    p.ped_inv_res = plan_pow2(p.ped_res) ? 1.0 / p.ped_res : 0.0;
    p.n_sub = plan_n_sub((double)c.step_hz);

    size_t max_stride = WAVE;
    p.big_view = false;
    for (const RobotClassHost& k : rcls) {
        if (!k.ok) REFUSE(IMGENV_EINVAL, "laser ray tables overflow their packing (too many beams x view cells)");
        p.big_view = p.big_view || k.big;
        max_stride = std::max(max_stride, (size_t)k.ray_stride);
    }
    if (rcls.size() > RC_INLINE || pcls.size() > PC_INLINE)
        REFUSE(IMGENV_EINVAL, "more than %d robot or %d pedestrian classes (shape, size, sensor) in one world", RC_INLINE, PC_INLINE);
    if (p.big_view)
        for (const RobotClassHost& k : rcls)
            if (!k.big) REFUSE(IMGENV_EINVAL, "robot classes with and without big views in one world");
    p.out = out_facts(c, g.Hv, g.Wv, g.B, p.RL);
    p.arena = plan_arena(p.out);
    p.full_rewrite = (c.flags & IMGENV_FLAG_FULL_REWRITE) != 0;
    if (p.full_rewrite && p.RL != p.R)  // (a shard's caller all-gathers the records in place: that buffer cannot be a copy)
        REFUSE(IMGENV_EINVAL, "IMGENV_FLAG_FULL_REWRITE is not available in a robot shard");
    if (c.out_arena && c.out_arena_bytes < (int64_t)p.arena.total)
        REFUSE(IMGENV_EINVAL, "out_arena too small: %lld < %zu", (long long)c.out_arena_bytes, p.arena.total);

    p.layer = plan_layer_mode(p.R, p.RL, p.P, W, Hg, Wg, c.flags, rcls, pcls);
    {   // k_raster's LDS box and the per-robot footprint cell lists (classes with a huge footprint go without)
        int box = 1, cap = 1, max_rad = 0;
        for (const RobotClassHost& k : rcls) {
            max_rad = std::max(max_rad, k.box_rad);
            const int side = 2 * k.box_rad + 1;
            if (side * side > RASTER_BOX_CELLS) continue;
            box = std::max(box, side * side);
            cap = std::max(cap, std::min(side * side, k.fp.n()));
        }
        p.pd_cap = 0;
        if (p.layer.sum) {  // the pedestrians' boxes share the rasters' LDS, and every pedestrian keeps the list of the cells it counts itself on
            int pbox = 1;
            for (const PedClassHost& k : pcls) pbox = std::max(pbox, (2 * k.box_rad + 1) * (2 * k.box_rad + 1));
            p.pd_cap = pbox;
            box = std::max(box, pbox);
        }
        p.box_cells = box;
        p.fp_cap = cap;
        p.region_margin = (int)ceil(0.5 * sqrt((double)g.Hv * g.Hv + (double)g.Wv * g.Wv)) + max_rad + 3;
    }
    p.PP = plan_obs_slots(p.Pw);  // sort slots of k_obs: a power of two, 64 * E of them in registers up to 1024 pedestrians
    p.obs_E = plan_obs_E(p.PP);
    // (measured: 200 pedestrians 1 pass 101.8, 2-5 passes 94-96 us per headline step; 1000 pedestrians 1 / 3 / 6 / 12 passes 316 / 303 / 282 / 282 us per cfg-5 step, 294 with the full sort every step)
    p.obs_passes = p.obs_E >= 8 ? 6 : p.obs_E >= 2 ? 3 : 0;
    max_stride += 4;  // + the dummy beam of view cells that no beam crosses (kept a multiple of 16 bytes)
    p.hit_stride = (int)max_stride;
    p.lds_view = plan_lds_view((size_t)g.Hv * g.Wv, max_stride, g.Wv);
    p.lds_obs = plan_lds_obs(p.obs_E, p.PP, p.Pw);
    if (p.big_view) {  // k_beams_big: the occupied plane of the crop bitmap; k_taps_big: the hit words
        const size_t tiles = (size_t)rcls[0].big_ta * rcls[0].big_tb;
        p.big_words = (int)((tiles * 2 + 1 + 3) & ~(size_t)3);  // + the always-free word the padded path entries point at
        p.big_hit_stride = (g.B + 3 + 3) & ~3;  // B hit words, the dummy beam, the flag, the collision code
        p.big_full_chunks = (int)(((size_t)g.Hv * g.Wv + VBF_T * 4 - 1) / (VBF_T * 4));
        p.big_bits_in_lds = plan_big_bits_in_lds((size_t)p.big_words);
        p.lds_view_big = plan_lds_view_big((size_t)p.big_words);
        p.lds_view = 16;
        if (taps_lds_bytes(g.B) > LDS_MAX) REFUSE(IMGENV_EINVAL, "the hit words of %d beams do not fit the 160 KiB LDS", g.B);
    }
    if (p.lds_view > LDS_MAX || p.lds_obs > LDS_MAX)
        REFUSE(IMGENV_EINVAL, "view (%zu B) or pedestrian list (%zu B) does not fit the 160 KiB LDS", p.lds_view, p.lds_obs);
    // the social-force crowd a step ahead: one that ignores the robots depends on nothing of a step
    p.sfm_ahead = c.ped_scene_type == IMGENV_SCENE_PEDSIM && c.relation_ped_robo != 1 && p.Pw > 0 && !serial;
    p.early = plan_early_obs(serial, p.P, p.NA, p.sfm_ahead, p.beep_on, cfg_has_limiters(c), p.big_view, p.n_sub);
    return IMGENV_OK;
}
#undef REFUSE
