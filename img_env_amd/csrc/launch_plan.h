// launch_plan.h -- the launch-shape rules as pure functions: which kernel variant runs at which grid, block
// and LDS size, decided from plain facts about the handle (fixed at imgenv_create) and about the chain of launches in hand.
// Nothing of HIP in here: plain C++17, compiled by g++ for tests/host/launch_plan_check.cpp, which pins every threshold
// below with its two neighbours.  The launch functions of imgenv_hip.hip build the facts, ask for a plan and issue the
// launches in stream order; what is launched at what shape is decided here, and so are the ordering's decisions (which stream,
// which event, which buffer takes the turn: "ordering" below, pinned by tests/host/step_chain_check.cpp) -- the host code only
// executes them.
//
// Also the one home of the constants that both the kernels and these rules read, and of `pick`, the step from a plan's
// runtime selector to a template instantiation.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "../../include/imgenv.h"

// ---------------------------------------------------------------------------------------- shared constants
#define WAVE 64
#define INT_G 8        // lanes per robot in k_integrate
#define INT_ITEMS 32   // sin / cos pairs per robot: the sub-step headings, the new heading and its half
#define INT_ROBOTS 32  // robots per 256-thread block
#define VBC_T 256    // k_crop_big: up to 4 wavefronts
#define VBB_T 256    // k_beams_big: one beam per thread
#define VBT_T 256    // k_taps_big: one sensor_map pixel per thread (host_tables.h lists its chunks of this many pixels)
#define VBF_T 256    // k_fullview_big
#define STAMP_MAX_ROBOTS (1 << 19)
#define STAMP_TAGS 255
#define MAP_BLOCKS 8  // k_reset_apply: workgroups that restore one world's map
#define STACK_BLOCK 256
#define STACK_MAX_BLOCKS 2048
#define EP_BLOCK 256
#define EP_MAX_BLOCKS 1024
#define EPLOG_BLOCK 1024    // k_episode_log: ONE workgroup (its records are numbered by a running count), 16 wavefronts
#define FINAL_BLOCK 256     // k_final_obs: one lane per chunk of a captured row
#define FINAL_MAX_BLOCKS 1024
#define FINAL_MAX_FIELDS 18  // 11 fields of imgenv_out, 3 stacks, ped_vector_norm, the two normalised states (normalise.h)
#define ROLLOUT_BLOCK 256   // k_rollout: one lane per chunk of a stored row
#define ROLLOUT_MAX_BLOCKS 1024
#define ROLLOUT_MAX_FIELDS 9  // five single-frame fields, ped_vector_norm, three stacks
#define ROLLOUT_NORM_FIELDS 2  // norm_vector_states, norm_state_stack (normalise.h; their pointers are imgenv_normalise_out's)
#define ROLLOUT_TABLE_FIELDS (ROLLOUT_MAX_FIELDS + ROLLOUT_NORM_FIELDS)  // what a field table of k_rollout / k_rollout_gather holds: 11
#define GAE_BLOCK 64        // k_rollout_gae: one lane per local robot, one wavefront per block (4096 robots reach 64 CUs)
#define GAE_MAX_BLOCKS 1024
#define GAE_BATCH 4         // time steps whose loads a lane issues before it walks their dependent chain
#define MB_INDEX_BLOCK 256   // k_mb_count / k_mb_scatter (minibatch.h): one workgroup per tile, a lane per MB_LANE_FLAGS flags
#define MB_LANE_FLAGS 16     // one 16-byte load of is_clean per lane
#define MB_TILE (MB_INDEX_BLOCK * MB_LANE_FLAGS)  // 4096 flags
#define MB_SCAN_BLOCK 256    // k_mb_scan: ONE workgroup, MB_SCAN_BLOCK tile counts per round, a carry from round to round
#define MB_STATS_BLOCK 256   // k_mb_stats: one workgroup per MB_STATS_TILE positions of the valid list, MB_STATS_PER_LANE per lane
#define MB_STATS_PER_LANE 16
#define MB_STATS_TILE (MB_STATS_BLOCK * MB_STATS_PER_LANE)
#define MB_SHUFFLE_BLOCK 256 // k_mb_shuffle: one lane per position of `order`
#define MB_ROUNDS 6          // Feistel rounds of the shuffle's permutation
#define SEQ_FLAG_BLOCK 256   // k_seq_flag (sequences.h): one lane per sequence
#define SEQ_MAX_STATES 2     // caller state arrays a sequence gather carries (IMGENV_SEQ_MAX_STATES)
#define SEQ_MAX_STATE_BYTES 65536
#define PED_DRAW_BLOCK 256       // k_ped_draw (ped_draw.h): one workgroup per drawn map, four wavefronts
#define PED_DRAW_MAX_BLOCKS 2048 // eight workgroups per CU of 256; the kernel strides over further rows
#define PED_DRAW_LDS_BYTES 65536 // the rank plane, a word per cell: 128 x 128 cells at most (96 x 96 takes 36 864 bytes)
#define NORM_BLOCK 256       // k_norm_part / k_norm_apply (normalise.h): four wavefronts, a lane per (row, column)
#define NORM_PER_LANE 8      // k_norm_part: the rows of a tile whose samples a lane holds in registers
#define NORM_MAX_COLS 64     // state_dim + 1 (the return) columns at most: the columns of a row lie in one wavefront
#define NORM_MAX_BLOCKS 1024
#define ACT_BLOCK 256       // k_actions: one lane per local robot
#define POL_BLOCK 256       // k_policy (policy.h): a group of 1, 4, 16 or 64 lanes per local robot
#define POL_REG 16          // logits a lane of k_policy keeps in registers; a longer block of the row is re-read
#define OBS_POST_BLOCK 256  // k_obs_post: one lane per element of a robot's ped_vector row
#define OBS_POST_MAX_BLOCKS 2048
#define TRACKS_BLOCK 256    // k_tracks_install: one workgroup per world of the chain
#define ORCA_NEAR_CAP 64  // robot agents a pedestrian can have within its 0.5 m neighbour range before k_orca falls back to the full scan
#define ORCA_MAX_ON 118   // obstacle neighbours kept per agent
#define ORCA_MAX_AN 10    // rvoscene.h:57,63 maxNeighbors
#define ORCA_MAX_LINES (ORCA_MAX_ON + ORCA_MAX_AN)
#define ORCA_STACK 128
#define ORCA_GROUP_MAX 4
#define ORCA_ROW 16
#define SFM_MAX_AGENTS 256
#define OWNER_MULTI 0xFFFFFEu  // 24-bit owner field of the composed layer: several robots cover the cell
#define RC_INLINE 6           // distinct robot classes (shape, size, sensor) per world, carried in the kernel arguments
#define PC_INLINE 4           // distinct pedestrian classes per world
#define RASTER_BOX_CELLS 2048  // LDS box of a robot raster: up to 45 x 45 cells

enum { LAYER_COMPOSED = 0, LAYER_STAMP = 1, LAYER_SUM = 2 };  // the class layer's mode (world.h), as the kernels take it

// ---------------------------------------------------------------------------------------- from selector to instantiation
// pick(f, a, b, ...) calls f(A, B, ...) with every runtime selector turned into a compile-time constant: a bool into
// std::true_type / std::false_type, a OneOf<V0, V1, ...>{v} into std::integral_constant<int, Vk> for the Vk that equals v
// (the LAST of the list when none does).  Each kernel family with more than two variants has one function that names its
// instantiations through this (imgenv_hip.hip: k_view_for, ...); launches and imgenv_create's LDS attributes both go through
// that function, so what gets the attribute is what can be launched.
template <int... Vs>
struct OneOf {
    int v;
};
template <class F>
inline void pick(F&& f) {
    f();
}
template <class F, class... Rest>
inline void pick(F&& f, bool b, Rest... rest);
template <class F, int V0, int... Vs, class... Rest>
inline void pick(F&& f, OneOf<V0, Vs...> o, Rest... rest) {
    if constexpr (sizeof...(Vs) > 0) {
        if (o.v != V0) return pick(f, OneOf<Vs...>{o.v}, rest...);
    }
    pick([&](auto... cs) { f(std::integral_constant<int, V0>{}, cs...); }, rest...);
}
template <class F, class... Rest>
inline void pick(F&& f, bool b, Rest... rest) {
    if (b) return pick([&](auto... cs) { f(std::true_type{}, cs...); }, rest...);
    pick([&](auto... cs) { f(std::false_type{}, cs...); }, rest...);
}

// ---------------------------------------------------------------------------------------- facts
// what imgenv_create fixes (imgenv_stack_enable / imgenv_episodes_enable add nothing here: their chunking is an argument)
struct PlanHandle {
    int R = 0, RL = 0, P = 0, W = 1, Rw = 0, Pw = 0, NA = 0;  // robots, local robots, pedestrians, worlds, per world, RVO agents
    bool sharded = false, sum_shard = false;                    // a robot shard; ... in SUM mode (world.h)
    bool pow2 = false;                                          // the resolution is an exact power of two
    int layer = LAYER_COMPOSED;
    bool serial = false;                                        // IMGENV_SERIAL=1: no side streams
    bool big_view = false, view_a4 = false;                     // view_big.h's kernels; Wv % 4 == 0
    int B = 0;                                                  // beams
    size_t lds_view = 0, lds_obs = 0, lds_view_big = 0;
    int obs_E = 0, n_sub = 0, relation = 0, scene = 0;
    bool early = false, gates_work = false;
    size_t Gs = 0;                                              // cells of one world's grid layer
    int box_cells = 0;                                          // the rasters' LDS box
    // plan_raster_pack: robot classes of the handle; every one has lattice rows and a box within box_cells; the largest footprint
    // bitmap (cells); IMGENV_RASTER_PACK as the handle's creation found it (-1: unset)
    int robot_classes = 0;
    bool pack_rows = false;
    int pack_bitmap_cells = 0;
    int pack_force = -1;
    int obs_room_force = -1;                                    // plan_obs_lds: IMGENV_OBS_ROOM as the handle's creation found it (-1: unset)
    int big_max_crop = 1, big_full_chunks = 1, big_tap_chunks_dyn = 0;
    bool big_bits_in_lds = true, crop_map = false;
    int img_w = 0, img_h = 0;
    bool resize = false, keep_view_maps = false;
};
// what the chain of launches in hand adds
struct PlanChain {
    int act_ng = 0, act_np = 0, act_nl = 0, act_nw = 0;  // robots, pedestrians, local robots, worlds the chain covers
    size_t act_cells = 0;
    bool listed = false;      // a world list is in use ...
    bool n_dev = false;       // ... whose length only the device knows (act_n_dev): grids by every world, variants by act_hint
    int act_hint = 0;
    bool is_reset = false, moved = false, local_only = false;
    unsigned stamp_seq = 0;
    int orca_cap = 1;         // the largest obstacle table any world of the handle can hold
    // what imgenv_step_begin reads
    bool chain_open = false, orca_ran = false, view_ran = false, in_step = false, comm = false, crowd_ahead = false;
    bool early_off = false;   // IMGENV_EARLY_OBS=0 (measurement switch)
};
struct LaunchShape {
    unsigned grid = 0, block = 0;
    size_t lds = 0;
};

// the count a variant is chosen by: what the launch covers, or what a device-side reset chain is expected to cover
inline int plan_by_hint(const PlanChain& c, int n) { return c.n_dev ? std::min(n, c.act_hint) : n; }
// k_integrate's LDS table of headings holds the step's sub-steps; otherwise k_integrate_serial, no fused move, no early step
inline bool plan_integrate_fits(int n_sub) { return n_sub >= 1 && n_sub + 2 <= INT_ITEMS; }
// the pedestrians move in the step's move launch (k_integrate, k_move_raster): RVO and recorded crowds; a social-force crowd has moved in k_sfm
inline bool plan_peds_move(const PlanHandle& h) { return h.P > 0 && (h.NA > 0 || h.scene == IMGENV_SCENE_DATASET); }
// k_compose / k_cell_base: 4 cells per thread over everything, or a fixed number of 256-thread blocks per listed world
inline unsigned plan_compose_blocks(const PlanHandle& h, const PlanChain& c) {
    return c.listed ? (unsigned)(((h.Gs / 4 + 255) / 256) * c.act_nw) : (unsigned)((c.act_cells / 4 + 255) / 256 + 1);
}

// ---------------------------------------------------------------------------------------- imgenv_create
// STAMP mode of the class layer instead of two owner layers + k_compose.  Composed wins where the agents cover a good part of
// the map (the headline world: 0.133 against 0.138 ms per step), stamped where the maps are much larger than what the agents
// touch (8192 one-robot worlds: 52 against 43 M robot-steps/s) -- measured: composed wins at 277 cells per agent, stamped at 1000
// ... and handles whose rasters and views are single small launches (at most 1024 blocks: bound by launch latency, not by
// their work) are better off without the k_compose launch however dense they are (cfg-2, 1024 robots at 156 cells per
// agent: 38.8 -> 36.3 us per step)
inline bool plan_layer_stamp(bool owns_all, size_t cells, int R, int P, uint32_t flags) {
    bool stamp = owns_all && cells > (size_t)512 * (R + P);
    if (owns_all && R + P <= 1024) stamp = true;
    if (flags & IMGENV_FLAG_COMPOSE_DENSE) stamp = false;
    if ((flags & IMGENV_FLAG_COMPOSE_SPARSE) && owns_all) stamp = true;
    if (stamp && R >= STAMP_MAX_ROBOTS) stamp = false;
    return stamp;
}
// sort slots of k_obs: a power of two, 64 * E of them in registers up to 1024 pedestrians (E = 0: LDS sort)
inline int plan_obs_slots(int Pw) {
    int PP = WAVE;
    while (PP < Pw) PP <<= 1;
    return PP;
}
inline int plan_obs_E(int PP) { return PP <= 1024 ? PP / WAVE : 0; }
// k_view: src u8 (+ dummy cells) | hit u32 | column terms | cursors of the final pass | largest hit step of blocks of beams (3 levels)
inline size_t plan_lds_view(size_t view_cells, size_t hit_stride, int Wv) {
    return ((view_cells + 16) & ~(size_t)15) + 4 * hit_stride + 16 * (size_t)Wv + 16 + 4 * (2 * (hit_stride / 8 + 1) + 4);
}
// k_view step (5): the room its resolve has in LDS that is dead by then, for a view of NC cells in rows of Wv whose final pass left
// n_skip entries in the skip list -- cap_d chunk descriptors (8 bytes each) behind the list, in what remains of the crop's
// ((NC + 16) & ~15) bytes, and cap_r result slots (4 bytes each) in the column table's 16 Wv bytes.  A cell that finds no room
// walks its list alone.  tiny: the -DIMGENV_EXP_TINY_RESOLVE build (exp_hooks.h), where nearly every cell does.
// (constexpr: the kernel calls it too; tests/host/k_view_resolve_room_check.cpp replays step (5) with these and smaller caps)
struct ResolveRoom {
    int cap_d, cap_r;
};
inline constexpr int plan_resolve_cap_d(int NC, int n_skip, bool tiny) { return tiny ? 5 : (((NC + 16) & ~15) / 4 - ((n_skip + 1) & ~1)) / 2; }
inline constexpr int plan_resolve_cap_r(int Wv, bool tiny) { return tiny ? 2 : 4 * Wv; }
inline constexpr ResolveRoom plan_resolve_room(int NC, int Wv, int n_skip, bool tiny = false) {
    return ResolveRoom{plan_resolve_cap_d(NC, n_skip, tiny), plan_resolve_cap_r(Wv, tiny)};
}
inline size_t plan_lds_obs(int obs_E, int PP, int Pw) {
    return (obs_E == 0 ? (size_t)PP * 8 : 0) + (size_t)(Pw > 0 ? Pw : 1) * 8 + (size_t)PP * 4 + WAVE * 7 * 4 + 16;
}
// k_beams_big: the occupied plane of the crop bitmap next to the hit words; beyond 150 KiB (views above ~1000 x 1000 cells) the
// beams read the bitmap from HBM
inline bool plan_big_bits_in_lds(size_t big_words) { return 4 * big_words <= 150 * 1024; }
inline size_t plan_lds_view_big(size_t big_words) { return (plan_big_bits_in_lds(big_words) ? 4 * big_words : 0) + 16; }
inline size_t plan_lds_fullview(int B) { return 16 * (size_t)((B + 4) / 4); }  // k_fullview_big: hit words (+ the dummy beam)
// k_taps_big: hit words (+ the dummy beam) | 16 tap values per pixel | list of the taps that need a second look | counter
inline size_t taps_lds_bytes(int B) { return plan_lds_fullview(B) + 16 * (size_t)VBT_T + 2 * 16 * (size_t)VBT_T + 16; }
inline constexpr size_t LDS_DEFAULT_MAX = 64 * 1024, LDS_MAX = 160 * 1024;  // above the first a kernel needs hipFuncAttributeMaxDynamicSharedMemorySize

// ---------------------------------------------------------------------------------------- step entry (imgenv_step_begin)
struct StepPlan {
    // the move is left to the raster launch (k_move_raster): launch_views', or -- sum_shard_now -- this call's own, over the shard's
    // robots and the pedestrians, in front of the exchange
    bool fuse_move = false, sum_shard_now = false;
    bool early_step = false;   // k_obs goes out with the move, behind a gate, instead of behind it (world.h)
    bool serial_move = false;  // k_integrate_serial
    int nb_robot = 0;          // the robots' blocks of the move; the pedestrians' follow
    LaunchShape move;
    bool fork_on_move = false;  // ev_fork rides on k_integrate's dispatch packet
};
inline StepPlan plan_step(const PlanHandle& h, const PlanChain& c) {
    StepPlan s;
    const bool fits = plan_integrate_fits(h.n_sub);
    // (a robot shard in SUM mode draws its own robots in this call anyway: the move goes into that launch, whoever runs the exchange)
    const bool whole_call = c.in_step && !h.sharded && !c.comm && h.RL == h.R;  // imgenv_step on a handle that owns its world
    // (the move inside the raster launch of BIG handles, with the early observation gated on that launch, was measured again in round 6:
    // 95.0 -> 103.1 us per headline step, cfg-4 117-123 -> 126, cfg-5 280 -> 282: the move's serial chain in front of every robot's
    // raster costs more than the launch it saves)
    s.fuse_move = (whole_call || h.sum_shard) && fits && (h.P == 0 ? h.RL <= 4096 : h.RL <= 1024);
    s.sum_shard_now = s.fuse_move && h.sum_shard;
    // early-observation step: only where gates work (k_gate_probe), no chain is half-way, and the snapshots it reads exist -- an RVO
    // crowd's from the last solve, a social-force crowd a step ahead stands still during the step
    const bool crowd_ready = h.NA == 0 ? c.crowd_ahead : c.orca_ran;
    s.early_step = h.early && h.gates_work && !s.fuse_move && !c.chain_open && crowd_ready && c.view_ran && !c.early_off;
    if (s.fuse_move) return s;
    s.serial_move = !fits;
    const int per_block = fits ? INT_G * INT_ROBOTS : 128, robots = fits ? INT_ROBOTS : 128;
    s.nb_robot = (h.RL + robots - 1) / robots;
    // ... and the pedestrians' move (img_env.cpp:343-358) in the same launch
    const int nb_ped = plan_peds_move(h) ? (h.P + per_block - 1) / per_block : 0;
    s.move = {(unsigned)(s.nb_robot + nb_ped), (unsigned)per_block, 0};
    // (the fork of the side streams follows right behind the move, on its dispatch packet)
    s.fork_on_move = fits && h.P > 0 && !h.serial && !c.chain_open;
    return s;
}

// ---------------------------------------------------------------------------------------- rasters (launch_rasters)
// The rasters of a chain of launches (in front of them, in STAMP mode, every STAMP_TAGS steps the sweep): every robot of the launch
// and every pedestrian -- or, local_only (a step of a robot shard in SUM mode, world.h: sum_shard), this rank's robots and the
// pedestrians: the other ranks' robots follow behind the exchange (k_remote)
struct RasterPlan {
    int n_g = 0, n_p = 0;
    bool small = false, roomy = false;
    int split = 0;         // robots and pedestrians in blocks of their own: the robots' blocks (0: block b draws robot b AND pedestrian b)
    int nw = 1;            // wavefronts per block: 1 or 4
    bool move = false;     // k_move_raster instead of k_raster
    int move_peds = 0;
    LaunchShape launch;    // k_raster / k_move_raster <pow2, layer, nw>
    bool sweep = false;    // STAMP mode: k_cell_base drops all stamps before their tags come round again
    unsigned sweep_blocks = 0;
};
inline RasterPlan plan_rasters(const PlanHandle& h, const PlanChain& c) {
    RasterPlan r;
    r.n_g = c.local_only ? h.RL : c.act_ng;
    r.n_p = c.act_np;
    // STAMP mode: no compose.  A reset has given the worlds it covers their base classes together with their obstacle maps
    // (k_reset_apply, k_reset_obstacles); every STAMP_TAGS steps one sweep drops all stamps before their tags come round again.
    r.sweep = h.layer == LAYER_STAMP && !c.is_reset && c.stamp_seq % STAMP_TAGS == 0;
    r.sweep_blocks = plan_compose_blocks(h, c);
    const int n_blocks = std::max(r.n_p, r.n_g);
    // four wavefronts per robot / pedestrian when the launch cannot fill the machine (device-side auto-reset: by the expected
    // number of robots, the grid itself is sized for every world)
    r.small = plan_by_hint(c, n_blocks) <= 1024;
    // robots and pedestrians in blocks of their own while all of them fit the chip at once (8192 wavefronts): a robot and a
    // pedestrian one behind the other in one block is twice a block's chain of memory round trips
    // (1024 envs x (4 + 3): k_raster 34 -> 22 us; the headline's 8192 + 200 stay as they are: a second, nearly empty round)
    r.roomy = !r.small && r.n_g + r.n_p <= 8192;
    r.split = (r.small || r.roomy) && r.n_g > 0 && r.n_p > 0 ? r.n_g : 0;
    r.nw = r.small ? 4 : 1;
    // (k_move_raster: the step's move in the same launch -- the RVO / recorded pedestrians' too)
    r.move = c.moved;
    r.move_peds = plan_peds_move(h) ? 1 : 0;
    r.launch = {(unsigned)(r.split || r.move ? r.n_g + r.n_p : n_blocks), (unsigned)(r.nw * WAVE), 4 * (size_t)h.box_cells + 16};
    return r;
}

// k_raster_pack<pow2, RPW> in place of k_raster: RPW robots per wavefront, 64 / RPW lanes and an LDS box each, the pedestrians in
// the blocks behind.  plan_rasters stays the plan of everything this refuses.  What it takes: SUM counts of a handle that owns its
// whole world, a step over every world (no reset, no world list, no device-side count, the move not fused), ONE robot class --
// the kernel reads the class record with a scalar index -- that has lattice rows, a box within the handle's and a footprint
// bitmap of at most 64 / RPW cells, and RPW boxes of LDS that leave a compute unit its 32 wavefronts.
struct RasterPackPlan {
    int rpw = 0;         // 0: not packed (k_raster / k_move_raster as plan_rasters says)
    LaunchShape launch;  // k_raster_pack <pow2, rpw>
};
inline size_t plan_raster_pack_lds(const PlanHandle& h, int rpw) { return (size_t)rpw * (4 * (size_t)h.box_cells + 16); }
inline bool plan_raster_pack_fits(const PlanHandle& h, int rpw) {
    return (rpw == 2 || rpw == 4) && h.layer == LAYER_SUM && !h.sharded && !h.sum_shard && h.RL == h.R && h.robot_classes == 1 &&
           h.pack_rows && h.pack_bitmap_cells >= 1 && h.pack_bitmap_cells <= WAVE / rpw &&
           LDS_MAX / ((plan_raster_pack_lds(h, rpw) + 1279) / 1280 * 1280) >= 32;
}
inline RasterPackPlan plan_raster_pack(const PlanHandle& h, const PlanChain& c) {
    RasterPackPlan r;
    if (c.is_reset || c.listed || c.n_dev || c.moved || c.local_only || c.act_ng != h.R || c.act_ng < 1) return r;
    // The size rule: the launches plan_rasters calls neither small nor roomy (more blocks than the chip holds wavefronts: the
    // headline's 8192 + 200), where packing turns two rounds of wavefronts into one.
    // RPW: four.  The headline step, one box, the switch at 0 / 2 / 4 interleaved three times (profiles/raster_pack_ab.txt):
    // 87.8 / 87.6 / 88.0 us with k_raster, 85.8 / 85.2 / 85.7 with two robots per wavefront, 83.1 / 83.7 / 83.6 with four.
    // Not where only two fit (a bitmap of more than 16 cells: cfg-5, where the step is k_obs' 205 us whatever the rasters do --
    // 279.9-280.9 us per step with k_raster, 281.0-281.9 with two per wavefront), and not beside a social-force crowd (cfg-4, whose
    // k_sfm shares the chip with the rasters: 104.1 / 104.2 / 105.1 us with k_raster, 111.1 / 111.3 / 102.3 packed).
    const bool big = c.act_ng + c.act_np > 8192 && h.scene != IMGENV_SCENE_PEDSIM;
    int want = big && plan_raster_pack_fits(h, 4) ? 4 : 0;
    if (h.pack_force >= 0) want = h.pack_force;  // IMGENV_RASTER_PACK (measurement switch): 0 never, 2 / 4 on every eligible chain
    if (want == 0 || !plan_raster_pack_fits(h, want)) return r;
    r.rpw = want;
    r.launch = {(unsigned)((c.act_ng + want - 1) / want + c.act_np), WAVE, plan_raster_pack_lds(h, want)};
    return r;
}

// ---------------------------------------------------------------------------------------- side launches (launch_views, launch_obs)
struct OrcaLaunch {
    int G;          // agents per wavefront (1, 2 or 4: one row of 16 lanes each)
    int groups;     // wavefronts per world
    int cap_on;     // obstacle neighbours an agent's scratch holds (the handle's largest obstacle table, at most ORCA_MAX_ON)
    int cap_stack;  // tree levels its walk may stack up
    int stage_obst; // obstacle segments / nodes the LDS staging area holds (0: read them from HBM, everything on the home lane)
    int fold_side;  // handles of several worlds: this kernel also does k_side_robots' part for its world (a launch less per phase):
                    // the world's robot agents out of the robot records (setRobotPos, img_env.cpp:411-417), Agent::get_state of
                    // its robots (group 0), and the robots taken as neighbour candidates directly instead of through near lists
    int zero_vel;   // (with fold_side) a reset: robot agents start at rest
};
// The pedestrian half of the observation needs the local robots' new poses only, so it starts right behind k_integrate (in a
// sharded world: underneath the record exchange) on its own stream; beside the rasters, compose and view run, on two side
// streams, that and the next step's _step_ped_normal solve (img_env.cpp:304-343).
struct SidePlan {
    bool remote_only = false;     // a robot shard in SUM mode has drawn its own robots in imgenv_step_begin: k_remote draws the other ranks'
    LaunchShape remote;
    bool side_reads_all = false;  // the side streams read the OTHER ranks' robots: their RVO agents (k_side_robots, k_orca)
    bool overlap = false, one_side = false;
    bool fold_side = false;       // k_orca does k_side_robots' part for its world itself (one launch less per phase)
    int rvo_agents = 0, slices = 1;
    LaunchShape robots;           // k_side_robots (unless fold_side)
    bool orca = false;
    OrcaLaunch L = {};
    unsigned orca_blocks = 0;     // (its LDS: orca_lds_bytes(L), kernels.h -- sized by the device's record types)
    bool state = false;           // no side streams: after a reset Agent::get_state gets its own small launch (in a step k_integrate
    LaunchShape state_shape;      // does it, with pedestrians k_side_robots)
};
inline SidePlan plan_side(const PlanHandle& h, const PlanChain& c) {
    SidePlan s;
    s.remote_only = h.sum_shard && !c.is_reset;
    s.remote = {(unsigned)((h.R - h.RL + 255) / 256), 256, 0};
    s.side_reads_all = h.P > 0 && h.NA > 0 && h.relation == 1;
    s.state = h.P == 0 && c.is_reset;
    s.state_shape = {(unsigned)((c.act_nl + 127) / 128), 128, 0};
    if (h.P == 0) return s;
    // (IMGENV_SERIAL=1 in the environment keeps everything on the caller's stream: clean per-kernel timings.)
    s.overlap = !h.serial;
    // Handles of at most 4096 robots keep ONE side stream: observation, robot records and the solve one behind the other (they
    // fit underneath the rasters + views with room to spare: 31 us against 72 at 1024 envs x (4 + 3)), which saves three of the
    // seven event operations of a phase -- such shapes are bound by the host's call rate (tools/host_issue_probe.py:
    // ~6 us per launch or event call, ~30 calls per step with a device-side reset)
    s.one_side = s.overlap && !h.sharded && h.RL <= 4096;
    // handles of several worlds with RVO crowds: k_orca does k_side_robots' part for its world itself (one launch less per phase)
    s.fold_side = h.W > 1 && h.NA > 0;
    // (slices of >= 48 pedestrians, four at most: 8192 robots x 200 pedestrians = 128 x 4 wavefronts.  More of them -- cfg-5's
    // 1000 pedestrians in 16 slices -- only take issue slots from the rasters and the views: 281-286 us per step against 276-278)
    s.rvo_agents = h.NA > 0 && h.relation == 1 ? 1 : 0;
    s.slices = s.rvo_agents && h.W == 1 ? std::min(4, std::max(1, (h.P + 47) / 48)) : 1;
    s.robots = {(unsigned)((c.act_ng + WAVE - 1) / WAVE) * (unsigned)s.slices, WAVE, 0};
    s.orca = h.NA > 0;
    if (s.orca) {
        // groups of up to 4 pedestrians of one world per wavefront; an agent's LDS scratch sized by the largest obstacle table
        // any world of the handle can hold, the table itself staged into LDS when it fits 256 segments
        const int per_world = h.W > 1 ? h.Pw : h.P, cap = std::max(c.orca_cap, 1);
        s.L.G = per_world > 2 ? ORCA_GROUP_MAX : per_world;  // a row of 16 lanes per agent
        s.L.groups = (per_world + s.L.G - 1) / s.L.G;
        s.L.cap_on = std::max(std::min(ORCA_MAX_ON, cap), ORCA_ROW - ORCA_MAX_AN);  // (a round's 16 candidate lines borrow the projection area)
        s.L.cap_stack = std::min(ORCA_STACK, cap + 1);
        s.L.fold_side = s.fold_side ? 1 : 0;
        s.L.zero_vel = c.is_reset ? 1 : 0;
        s.L.stage_obst = std::min(cap, 256);  // (a world with more segments than that is solved out of HBM: the kernel checks its count)
        s.orca_blocks = (unsigned)((c.act_np / per_world) * s.L.groups);
    }
    return s;
}
// k_obs<E>: a wavefront per local robot
// (four wavefronts per robot for 513 .. 1024 pedestrians -- three times the occupancy, a third of the LDS per wavefront --
// were measured in round 6 and LOSE: cfg-5 277 -> 325 us per step, 321 with two, 406 with eight: the step is bound by the
// instructions it issues, k_obs beside k_view, not by this kernel's occupancy.  docs/HISTORY.md)
//
// Room for the packed rasters beside an early k_obs: k_obs goes out first and fills the chip -- its 4.4 KB of LDS round up to four
// 1280-byte granules, 32 wavefronts of it are a compute unit's whole 160 KiB -- and the raster launch behind it (2048 + 200
// wavefronts at the headline shape, nine per compute unit) gets a wavefront slot, registers and LDS only as k_obs' wavefronts
// retire.  A k_obs workgroup that asks for more LDS than it uses keeps fewer of itself on a compute unit.  plan_obs_lds answers
// the smallest size, in granules, at which a compute unit full of k_obs workgroups still has `room` wavefront slots AND `room`
// times the raster's LDS free; lds_obs itself where nothing is packed behind the observation (raster_blocks 0), where the switch
// says 0, or where no size does it.  What a compute unit holds is floor(128 granules / size), so the steps are coarse: with the
// headline's sizes (four granules, one per raster workgroup) room 1-3 gives five granules (25 k_obs workgroups, three granules
// left over), room 4-8 ten (12 and 8), room 9 thirteen (9 and 11).
// room_force: IMGENV_OBS_ROOM as the handle's creation found it (measurement switch; -1: unset, the rule's own value).
// The rule's own value: OBS_ROOM_RULE workgroups, the first step.  The headline step, one box, the switch at 0 / 2 / 4 / 9 interleaved
// three times (profiles/raster_chain_ab.txt): 82.0 / 82.5 / 81.3 us per step with k_obs as it was, 79.8 / 80.0 / 80.3 at five
// granules (k_obs itself 32.6 -> 37.4 us by HIP events, the step ends earlier all the same), 96.2 / 96.4 / 96.5 at ten and
// 105.3 / 105.3 / 104.2 at thirteen, where k_obs (51-53 and 70-72 us) has become the step's longest chain.
#define OBS_ROOM_RULE 2
inline size_t plan_obs_lds(size_t lds_obs, unsigned raster_blocks, size_t raster_lds, int room_force) {
    const int room = room_force >= 0 ? room_force : OBS_ROOM_RULE;
    if (raster_blocks == 0 || room <= 0 || room >= 32) return lds_obs;
    const size_t cu = LDS_MAX / 1280, need = (size_t)room * ((raster_lds + 1279) / 1280);
    for (size_t g = std::max<size_t>((lds_obs + 1279) / 1280, 1); g <= cu; g++) {
        const size_t n = std::min<size_t>(cu / g, 32);  // k_obs workgroups (one wavefront each) a compute unit holds at this size
        if (32 - n >= (size_t)room && cu - n * g >= need) return g * 1280;
    }
    return lds_obs;
}
// (early_step: plan_step's, of the step this observation belongs to -- the rasters it shares the chip with are that step's)
inline LaunchShape plan_obs(const PlanHandle& h, const PlanChain& c, bool early_step = false) {
    const RasterPackPlan k = early_step ? plan_raster_pack(h, c) : RasterPackPlan{};
    return {(unsigned)c.act_nl, WAVE, plan_obs_lds(h.lds_obs, k.rpw ? k.launch.grid : 0u, k.launch.lds, h.obs_room_force)};
}

// ---------------------------------------------------------------------------------------- ordering (launch_views, imgenv_step_begin)
// The side wiring of a chain with pedestrians: one fork and one join per step on the caller's stream (every event operation costs
// it a ~6 us dependency bubble).  The observation's stream finally waits for the solve, so its join event covers both.
enum { ON_CALLER = 0, ON_SIDE = 1, ON_SIDE2 = 2 };      // a stream: the caller's, imgenv::side, imgenv::side2
enum { WAIT_NONE = 0, WAIT_FORK = 1, WAIT_FORK2 = 2 };  // what a side launch waits for: nothing, ev_fork, ev_fork2
struct SideWiring {
    int solve_on = ON_CALLER, obs_on = ON_CALLER;  // k_side_robots + k_orca; k_obs
    // the solve's wait: ev_fork where it has a stream of its own -- or shares the observation's and that went out with the step, in
    // front of the move (an early step) --, ev_fork2 where it needs every rank's robots: a second fork behind the exchange ...
    int solve_waits = WAIT_NONE;
    bool record_fork2 = false;     // ... recorded on the caller's stream in front of the wait,
    bool fork2_on_remote = false;  // or riding on k_remote's dispatch packet (a robot shard in SUM mode)
    bool join = false;             // ev_join behind the solve, the observation's stream waits for it
    bool join2 = false;            // ev_join2 behind the observation; the caller's stream waits for it behind the views
};
inline SideWiring plan_side_wiring(const SidePlan& s, const PlanHandle& h, bool early_step) {
    SideWiring w;
    w.fork2_on_remote = s.remote_only && s.side_reads_all && !h.serial;
    if (!s.overlap) return w;
    w.solve_on = s.one_side ? ON_SIDE2 : ON_SIDE;
    w.obs_on = ON_SIDE2;
    if (s.one_side)
        w.solve_waits = early_step ? WAIT_FORK : WAIT_NONE;  // (behind k_obs in its stream otherwise)
    else
        w.solve_waits = h.sharded && s.side_reads_all ? WAIT_FORK2 : WAIT_FORK;
    w.record_fork2 = w.solve_waits == WAIT_FORK2 && !s.remote_only;
    w.join = !s.one_side;
    w.join2 = true;
    return w;
}

// The snapshots the next step's early k_obs reads (world.h: ped_snap behind k_orca, rec_snap behind k_view).  A launch over every
// world writes one buffer and the next one the other; a launch over a world list -- a reset chain, nothing else is in flight --
// writes both and does not take a turn.  -1: no buffer.  An early step reads what the last turn wrote.
struct SnapTurn {
    int out = -1, out2 = -1;
    bool advance = false;
};
inline SnapTurn plan_snap_turn(unsigned seq, bool early, bool listed) {
    return {early ? (int)(seq & 1) : -1, early && listed ? (int)((seq + 1) & 1) : -1, !listed};
}
inline int plan_snap_in(unsigned seq) { return (int)((seq - 1) & 1); }

// The running normalisation of a chain (normalise.h): with training on the chain's batch goes into the statistics -- a reset
// chain has no return column -- then every chain applies them to the rows it covers (a reset chain of a reward-only handle in
// evaluation has nothing to do).
struct NormChain {
    int n_ret = 0, cols = 1, update = 0;  // NormDev's fields of this launch
    bool part = false, apply = false;     // k_norm_part, k_norm_apply
    bool turn = false, ret_turn = false;  // norm_turn / norm_ret_turn advance
};
inline NormChain plan_norm_chain(bool training, bool reward, int n_obs, bool is_reset) {
    NormChain n;
    n.n_ret = !is_reset && reward ? 1 : 0;
    n.cols = std::max(1, n_obs + n.n_ret);
    n.update = training ? 1 : 0;
    n.part = n.turn = training && (!is_reset || n_obs > 0);
    n.apply = !is_reset || n_obs > 0 || (training && reward);
    n.ret_turn = training && n.n_ret;
    return n;
}

// A step of the social-force crowd (sfm.h).  A crowd that runs a step ahead (imgenv_hip.hip: CrowdAhead, step_crowd): this step's
// state is in the other set -- swap the sets and publish -- or, behind a reset, is computed now, in place.
// Ordering against the caller's stream.  The launch ahead reads the live set and WRITES the other one -- the set that was live a
// step ago, which THAT step's k_sfm_publish (or in-place step) touched on the caller's stream.  Nothing else orders the crowd's
// stream behind the caller's: a host that queues steps faster than the device drains them (an asynchronous trainer, bench.py's
// timed loop) would let the crowd run several steps ahead and overwrite a set before it has been published (rounds 3-5 did).  So
// every step leaves an event behind its access to the sets on the caller's stream, by step parity (ev_in[leaves]), and the launch
// ahead waits for the LAST step's -- this step's publish only reads the live set, as the launch ahead does, so the crowd may run
// up to one step ahead of the caller's stream -- or for this step's own when it wrote the live set in place.
// No launch ahead in the first step behind a reset: a handle whose worlds are reset every other step -- many small worlds with
// their own time limits -- would compute ahead what the next reset drops, and make that reset wait for it.
// A crowd that cannot run ahead steps in place and leaves nothing.
struct CrowdStep {
    bool swap = false;     // swap the sets and k_sfm_publish; otherwise k_sfm in place
    int leaves = -1;       // CrowdAhead::ev_in[.] recorded behind this step's access (-1: none)
    int ahead_waits = -1;  // CrowdAhead::ev_in[.] the launch ahead waits for (-1: no launch ahead)
    int par_next = 0;
};
inline CrowdStep plan_crowd_step(bool ahead, bool ahead_valid, int steps_since_reset, int par) {
    CrowdStep k;
    k.par_next = par;
    if (!ahead) return k;
    k.swap = ahead_valid;
    k.leaves = par;
    k.par_next = par ^ 1;
    if (steps_since_reset >= 1) k.ahead_waits = k.swap ? par ^ 1 : par;
    return k;
}

// ---------------------------------------------------------------------------------------- views (launch_views)
struct ViewPlan {
    // k_view <pow2, a4, stamp, nw>
    bool lds_bound = false;
    int nw = 1;  // wavefronts per view: 1, 2, 4 or 8
    LaunchShape view;
    // view_big.h: crop (tiles of every robot spread over the chip) -> beams (a workgroup per robot and 256 beams) -> the shrunk
    // sensor_map (a thread per pixel) -> the full view, only where it is an output
    int quarters = 0, tap_chunks = 0;
    int tpw = 0, crop_chunks = 0;  // tiles per k_crop_big wavefront; its chunks per robot
    int qpw = 0;                   // blocks of 256 beams per k_beams_big workgroup
    int crop_sel = 0;              // k_crop_big: 0 <false, false>, 1 <STAMP, false>, 2 <STAMP, crop_map>
    bool taps = false, full = false, listed = false;
    int tap_wgs = 0;
    LaunchShape crop, beams, taps_shape, fullview;
};
// one wavefront per robot when the launch fills the machine, four when it is small (a reset of a few worlds): then
// the single wavefront's latency is all there is
// ... and whenever a view's LDS (crop + hit words + column table: 15 KB at 96 x 96 cells and 720 beams) would leave a
// compute unit with 16 or fewer one-wavefront workgroups -- four or fewer wavefronts per SIMD where the registers allow
// eight: four wavefronts then share one view's LDS (cfg-5, 8192 robots: k_view 252 -> 179 us alone, the step 472 -> 377 us;
// at 48 x 48 cells, 5 KB and 32 workgroups per unit, it loses: 63 -> 87 us)
inline bool plan_lds_bound(size_t lds_view) { return LDS_MAX / ((lds_view + 1279) / 1280 * 1280) <= 16; }
inline ViewPlan plan_views(const PlanHandle& h, const PlanChain& c) {
    ViewPlan v;
    const int n_l = c.act_nl, n_eff = plan_by_hint(c, n_l);
    if (!h.big_view) {
        v.lds_bound = plan_lds_bound(h.lds_view);
        // two wavefronts per robot in between (1025-4096 robots: every wavefront still resident at once; 1024 envs x 4: 39 -> 28 us)
        // ... and eight where a launch is at most 1024 robots and the view small (48 x 48 cells and 360 beams are then ONE round of groups
        // and ONE round of beams per wavefront: cfg-2 k_view 21.6 -> 20.4 us)
        v.nw = v.lds_bound ? 4 : n_eff <= 1024 ? 8 : n_eff <= 4096 ? 2 : 1;
        v.view = {(unsigned)n_l, (unsigned)(v.nw * WAVE), h.lds_view};
        return v;
    }
    v.quarters = std::max(1, (h.B + VBB_T - 1) / VBB_T);
    v.tap_chunks = (h.img_w * h.img_h + VBT_T - 1) / VBT_T;
    v.full = h.keep_view_maps || !h.resize;
    v.taps = h.resize;
    // tiles per wavefront: 8 while the launch is a handful of robots (a reset of a few worlds: every robot on ~40 workgroups), 32-64
    // once there are enough robots to fill the chip anyway
    // (measured again after the kernel's gathers stopped binding it: a wavefront's prologue -- pose, fixed-point terms, its tiles'
    // corner records -- is worth ~8 tiles, so even 256 robots want 32 tiles per wavefront: 36 -> 29 us; 2048 robots 64: 152 -> 133.
    // Handing the fixed-point terms over from the robot's raster instead of recomputing them per wavefront was measured too:
    // 155 us at 2048 robots, i.e. worse -- the prologue's cost is its loads, not its arithmetic.)
    v.tpw = n_eff >= 1024 ? 64 : n_eff >= 48 ? 32 : 8;
    v.crop_chunks = (h.big_max_crop + (VBC_T / WAVE) * v.tpw - 1) / ((VBC_T / WAVE) * v.tpw);
    // (2048 robots x 1000 beams: one block of 256 beams per workgroup 98 us, two 87, four 87 -- but end to end two win: 3.85 M robot-steps/s
    // against 3.79 / 3.78: the first workgroup of a robot also hands the collision code to the step's tail)
    v.qpw = n_eff >= 1024 ? std::min(2, v.quarters) : 1;
    v.crop_sel = h.layer == LAYER_STAMP ? (h.crop_map ? 2 : 1) : 0;
    v.crop = {(unsigned)((n_l + 7) / 8 * 8) * (unsigned)v.crop_chunks, VBC_T, 0};
    v.beams = {(unsigned)n_l * (unsigned)((v.quarters + v.qpw - 1) / v.qpw), VBB_T, h.lds_view_big};
    // (a step only runs the chunks of pixels a beam can reach: static list per class; the chunks behind the sensor hold their
    // 200 / 100 since the reset)
    v.listed = !c.is_reset && h.big_tap_chunks_dyn > 0 && h.big_tap_chunks_dyn < v.tap_chunks;
    v.tap_wgs = v.listed ? h.big_tap_chunks_dyn : v.tap_chunks;
    v.taps_shape = {(unsigned)n_l * (unsigned)v.tap_wgs, VBT_T, taps_lds_bytes(h.B)};
    v.fullview = {(unsigned)n_l * (unsigned)h.big_full_chunks, VBF_T, plan_lds_fullview(h.B)};
    return v;
}

// ---------------------------------------------------------------------------------------- chain tail: k_stack, k_episodes, k_obs_post
// A step covers every local robot; a reset chain the robots of its list's worlds, whose length the host knows (act_nw) or a
// kernel has counted (n_dev: the grid is sized for a guess and strides).
inline size_t plan_tail_rows(const PlanHandle& h, const PlanChain& c) {
    if (!c.is_reset || !c.listed) return (size_t)h.RL;
    return (size_t)(c.n_dev ? std::min(c.act_nw * h.Rw, std::max(c.act_hint, h.Rw)) : c.act_nw * h.Rw);
}
inline LaunchShape plan_tail(size_t items, int block, int max_blocks) {
    return {(unsigned)std::min<size_t>((size_t)max_blocks, std::max<size_t>(1, (items + block - 1) / block)), (unsigned)block, 0};
}
// `per_row` lanes per robot of the chain, striding over at most `max_blocks` blocks: k_stack its chunks_per_robot (STACK_BLOCK,
// STACK_MAX_BLOCKS), k_episodes one (EP_*), k_obs_post the 1 + 7 max_ped elements of a ped_vector row, or one where only
// close_to_human is kept (OBS_POST_*)
inline LaunchShape plan_tail_launch(const PlanHandle& h, const PlanChain& c, size_t per_row, int block, int max_blocks) {
    return plan_tail(plan_tail_rows(h, c) * per_row, block, max_blocks);
}

// k_episode_log (episode_log.h), in front of a reset chain's k_episodes<true>: one workgroup whatever the chain covers -- the
// records take their numbers from a count that runs through the block, chunk by chunk of EPLOG_BLOCK rows
inline LaunchShape plan_episode_log_launch() { return {1, EPLOG_BLOCK, 0}; }

// ---------------------------------------------------------------------------------------- head of a reset chain: k_final_obs
// k_final_obs (final_obs.h) copies the rows a reset chain is about to overwrite.  A row of a field is cut into chunks of `unit`
// bytes, the largest of 16 / 8 / 4 / 2 / 1 that divides the row's size (every base is 256-byte aligned, so a row starts on a
// multiple of its unit); one lane copies one chunk, a row of the launch is the sum of its fields' chunks.
struct FinalFieldPlan {
    uint32_t row_bytes = 0, unit = 1, chunks = 0;
};
inline FinalFieldPlan plan_final_field(size_t row_bytes) {
    FinalFieldPlan f;
    f.row_bytes = (uint32_t)row_bytes;
    f.unit = row_bytes % 16 == 0 ? 16 : row_bytes % 8 == 0 ? 8 : row_bytes % 4 == 0 ? 4 : row_bytes % 2 == 0 ? 2 : 1;
    f.chunks = (uint32_t)(row_bytes / f.unit);
    return f;
}
struct FinalPlan {
    FinalFieldPlan f[FINAL_MAX_FIELDS];
    int n_fields = 0;
    uint32_t chunks_per_row = 0;
    size_t bytes_per_row = 0;
};
// the table of the fields in hand, in the caller's order (n <= FINAL_MAX_FIELDS; fields of no bytes are refused by the caller)
inline FinalPlan plan_final_fields(const size_t* row_bytes, int n) {
    FinalPlan p;
    for (int k = 0; k < n && k < FINAL_MAX_FIELDS; k++) {
        p.f[p.n_fields] = plan_final_field(row_bytes[k]);
        p.chunks_per_row += p.f[p.n_fields].chunks;
        p.bytes_per_row += row_bytes[k];
        p.n_fields++;
    }
    return p;
}
// rows x chunks per row in blocks of FINAL_BLOCK, capped; the kernel strides.  The rows are the chain's (every local robot, or Rw
// per listed world); behind a device-side reset nobody on the host knows the count, and the grid is sized for `dev_guess` worlds --
// plan_dev_reset's guess from the same stale count its own grids use -- while the kernel reads the count on the device.
inline LaunchShape plan_final_obs_launch(const PlanHandle& h, const PlanChain& c, uint32_t chunks_per_row, int dev_guess) {
    size_t rows = (size_t)h.RL;
    if (c.listed) rows = (size_t)(c.n_dev ? std::min(c.act_nw, std::max(dev_guess, 1)) : c.act_nw) * (size_t)h.Rw;
    return plan_tail(rows * chunks_per_row, FINAL_BLOCK, FINAL_MAX_BLOCKS);
}

// ---------------------------------------------------------------------------------------- end of a chain: k_rollout, and k_rollout_gae
// k_rollout (rollout.h), the last launch of a chain: the rows are the chain tail's (plan_tail_rows), a row's chunks plan_final_field's,
// one lane per chunk, capped; the kernel strides.  The cap is reached from ROLLOUT_BLOCK x ROLLOUT_MAX_BLOCKS = 262144 chunks on.
inline LaunchShape plan_rollout_launch(const PlanHandle& h, const PlanChain& c, uint32_t chunks_per_row) {
    return plan_tail_launch(h, c, chunks_per_row, ROLLOUT_BLOCK, ROLLOUT_MAX_BLOCKS);
}
// imgenv_rollout_begin: every local row, whatever chain came last
inline LaunchShape plan_rollout_begin_launch(const PlanHandle& h, uint32_t chunks_per_row) {
    return plan_tail((size_t)h.RL * chunks_per_row, ROLLOUT_BLOCK, ROLLOUT_MAX_BLOCKS);
}
// the advantage pass: one lane per local robot, striding from GAE_BLOCK x GAE_MAX_BLOCKS = 65536 robots on
inline LaunchShape plan_rollout_gae_launch(const PlanHandle& h) { return plan_tail((size_t)h.RL, GAE_BLOCK, GAE_MAX_BLOCKS); }

// ---------------------------------------------------------------------------------------- behind the window: the minibatch kernels
// minibatch.h.  The index: one workgroup per tile of MB_TILE flags for the count and the scatter (no cap: 2^31 flags are 2^19
// workgroups), ONE workgroup for the scan in between.  The statistics: one workgroup per MB_STATS_TILE positions of the valid list
// (sized for all `flags`: nobody on the host knows how many are valid), ONE for each reduction.  The shuffle: a lane per position
// of `order`, all T x R of them.  The gather: k_rollout's walk over batch x chunks per row, capped; the kernel strides.
inline size_t plan_mb_tiles(size_t flags) { return (flags + MB_TILE - 1) / MB_TILE; }
inline LaunchShape plan_mb_index_launch(size_t flags) { return {(unsigned)std::max<size_t>(1, plan_mb_tiles(flags)), MB_INDEX_BLOCK, 0}; }
inline LaunchShape plan_mb_scan_launch() { return {1, MB_SCAN_BLOCK, 0}; }
inline size_t plan_mb_stats_tiles(size_t flags) { return (flags + MB_STATS_TILE - 1) / MB_STATS_TILE; }
inline LaunchShape plan_mb_stats_launch(size_t flags) { return {(unsigned)std::max<size_t>(1, plan_mb_stats_tiles(flags)), MB_STATS_BLOCK, 0}; }
inline LaunchShape plan_mb_stats_final_launch() { return {1, MB_STATS_BLOCK, 0}; }
inline LaunchShape plan_mb_shuffle_launch(size_t positions) {
    return {(unsigned)std::max<size_t>(1, (positions + MB_SHUFFLE_BLOCK - 1) / MB_SHUFFLE_BLOCK), MB_SHUFFLE_BLOCK, 0};
}
inline LaunchShape plan_mb_gather_launch(size_t batch, uint32_t chunks_per_row) {
    return plan_tail(batch * chunks_per_row, ROLLOUT_BLOCK, ROLLOUT_MAX_BLOCKS);
}
// sequences.h.  The flags: a lane per sequence, no cap (2^31 sequences are 2^23 workgroups).  The compaction and the shuffle are
// the minibatches' launches over the sequences.  The gather: length x batch x chunks per row field items, then batch x state chunks
// state items, capped; the kernel strides.
inline size_t plan_seq_chunks(size_t steps, size_t length) { return (steps + length - 1) / length; }
inline LaunchShape plan_seq_flag_launch(size_t sequences) {
    return {(unsigned)std::max<size_t>(1, (sequences + SEQ_FLAG_BLOCK - 1) / SEQ_FLAG_BLOCK), SEQ_FLAG_BLOCK, 0};
}
inline LaunchShape plan_seq_gather_launch(size_t length, size_t batch, uint32_t chunks_per_row, uint32_t state_chunks) {
    return plan_tail(length * batch * chunks_per_row + batch * state_chunks, ROLLOUT_BLOCK, ROLLOUT_MAX_BLOCKS);
}

// ---------------------------------------------------------------------------------------- anywhere: k_ped_draw
// ped_draw.h: one workgroup per map, capped -- the kernel strides -- with the map's rank plane, a word per cell, as dynamic LDS.  A
// pedestrian map whose plane is beyond PED_DRAW_LDS_BYTES cannot be drawn: imgenv_ped_maps_draw and IMGENV_ROLLOUT_PED_MAPS_DRAWN
// refuse it.
inline size_t plan_ped_draw_lds(int Hp, int Wp) { return (size_t)std::max(Hp, 0) * (size_t)std::max(Wp, 0) * 4; }
inline bool plan_ped_draw_fits(int Hp, int Wp) { return Hp >= 1 && Wp >= 1 && plan_ped_draw_lds(Hp, Wp) <= PED_DRAW_LDS_BYTES; }
inline LaunchShape plan_ped_draw_launch(size_t rows, int Hp, int Wp) {
    return {(unsigned)std::min<size_t>(PED_DRAW_MAX_BLOCKS, std::max<size_t>(1, rows)), PED_DRAW_BLOCK, plan_ped_draw_lds(Hp, Wp)};
}

// ---------------------------------------------------------------------------------------- chain tail: k_norm_part, k_norm_apply
// normalise.h.  A wavefront holds WAVE / cols whole rows, a lane per (row, column); a tile of k_norm_part is what a workgroup's
// lanes hold NORM_PER_LANE rows deep.  One workgroup per tile of the chain's rows, one per pass of the apply, both capped: the
// kernels stride over tiles / passes, and over whatever a device-side count turns out to be.
// (constexpr: the kernels call them too)
inline constexpr int plan_norm_rows_per_wave(int cols) { return WAVE / (cols > 1 ? cols : 1); }
inline constexpr size_t plan_norm_tile_rows(int cols) { return (size_t)(NORM_BLOCK / WAVE) * plan_norm_rows_per_wave(cols) * NORM_PER_LANE; }
inline constexpr size_t plan_norm_tiles(size_t rows, int cols) { return (rows + plan_norm_tile_rows(cols) - 1) / plan_norm_tile_rows(cols); }
inline LaunchShape plan_norm_part_launch(const PlanHandle& h, const PlanChain& c, int cols) {
    return {(unsigned)std::min<size_t>(NORM_MAX_BLOCKS, std::max<size_t>(1, plan_norm_tiles(plan_tail_rows(h, c), cols))), NORM_BLOCK, 0};
}
inline LaunchShape plan_norm_apply_launch(const PlanHandle& h, const PlanChain& c, int cols) {
    const size_t per_block = (size_t)(NORM_BLOCK / WAVE) * plan_norm_rows_per_wave(cols);
    return {(unsigned)std::min<size_t>(NORM_MAX_BLOCKS, std::max<size_t>(1, (plan_tail_rows(h, c) + per_block - 1) / per_block)), NORM_BLOCK, 0};
}

// ---------------------------------------------------------------------------------------- the features' device blocks
// A feature's arrays live in ONE zeroed allocation, every array on a 256-byte boundary (so a row of any field starts on a multiple
// of its unit).  The layouts are fixed here, device-free: the enable functions of imgenv_hip.hip allocate `total` bytes and hand
// out block + offset; tests/host/field_rows_check.cpp pins every offset of all seven (the stacks, the final observations, the
// rollout, the minibatches, the normalisation, the policy head, the PPO loss).
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
struct Carve {
    size_t total = 0;
    size_t take(size_t bytes) {  // the offset of the next array (one of no bytes takes no room: its offset is the next one's)
        const size_t at = total;
        total = align256(total + bytes);
        return at;
    }
};

// imgenv_stack_enable: the stacks of sensor_maps, vector_states, lasers, [RL][depth][frame]; a field of depth < 2 takes no room
struct StackPlan {
    int depth[3];          // effective depths (0 = not stacked)
    size_t frame_bytes[3];
    size_t off[3], total;
};
inline StackPlan plan_stack(size_t image_cells, int state_dim, int beams, int image_batch, int state_batch, int laser_batch, size_t RL) {
    StackPlan p;
    p.depth[0] = image_batch > 0 ? image_batch : 0;
    p.depth[1] = state_batch > 0 ? state_batch : 0;
    p.depth[2] = laser_batch >= 0 && beams > 0 ? std::max(laser_batch, 1) : 0;
    p.frame_bytes[0] = image_cells * 2;
    p.frame_bytes[1] = (size_t)state_dim * 4;
    p.frame_bytes[2] = (size_t)beams * 8;
    Carve c;
    for (int k = 0; k < 3; k++) p.off[k] = c.take(p.depth[k] >= 2 ? RL * p.depth[k] * p.frame_bytes[k] : 0);
    p.total = c.total;
    return p;
}

// imgenv_final_obs_enable: final_count [RL], then the n selected fields [RL][row bytes] in the caller's order
struct FinalObsLayout {
    size_t count, field[FINAL_MAX_FIELDS], total;
};
inline FinalObsLayout plan_final_obs_layout(const size_t* row_bytes, int n, size_t RL) {
    FinalObsLayout l = {};
    Carve c;
    l.count = c.take(4 * RL);
    for (int k = 0; k < n; k++) l.field[k] = c.take(RL * row_bytes[k]);
    l.total = c.total;
    return l;
}

// imgenv_rollout_enable (rollout.h has the shapes): per selected field its ring and its final list, then the transitions' arrays
struct RolloutLayout {
    size_t ring[ROLLOUT_TABLE_FIELDS], fin[ROLLOUT_TABLE_FIELDS];
    size_t actions, rewards, dones, is_clean, dones_info, final_idx, final_slot, final_row, final_n, total;
};
inline RolloutLayout plan_rollout_layout(const size_t* row_bytes, int n, size_t RL, size_t T, size_t F) {
    RolloutLayout l = {};
    Carve c;
    for (int k = 0; k < n; k++) {
        l.ring[k] = c.take((T + 1) * RL * row_bytes[k]);
        l.fin[k] = c.take(F * row_bytes[k]);
    }
    l.actions = c.take(T * RL * 12);
    l.rewards = c.take(T * RL * 4);
    l.dones = c.take(T * RL);
    l.is_clean = c.take(T * RL);
    l.dones_info = c.take(T * RL * 4);
    l.final_idx = c.take((T + 1) * RL * 4);
    l.final_slot = c.take(F * 4);
    l.final_row = c.take(F * 4);
    l.final_n = c.take(8);
    l.total = c.total;
    return l;
}

// imgenv_rollout_minibatch_enable (minibatch.h): the index, the statistics' scratch, then per gathered field and per scalar array
// its `buffers` copies side by side (one strided view covers a field's buffers)
enum { MB_S_ACTIONS, MB_S_REWARDS, MB_S_DONES, MB_S_DONES_INFO, MB_S_INDEX, MB_S_WEIGHT, MB_S_SCALARS, MB_S_COUNT };
struct MinibatchLayout {
    size_t valid, order, valid_n, norm, tile_count, tile_base, stat_part, stat_mean;
    size_t field[IMGENV_MB_MAX_BUFFERS][ROLLOUT_TABLE_FIELDS], scalar[IMGENV_MB_MAX_BUFFERS][MB_S_COUNT], total;
};
inline MinibatchLayout plan_minibatch_layout(const size_t* row_bytes, int n, size_t RL, size_t T, size_t batch, size_t buffers) {
    MinibatchLayout l = {};
    const size_t tiles = std::max(plan_mb_tiles(T * RL), plan_mb_stats_tiles(T * RL)), B = batch;
    Carve c;
    l.valid = c.take(T * RL * 4);
    l.order = c.take(T * RL * 4);
    l.valid_n = c.take(4);
    l.norm = c.take(8);
    l.tile_count = c.take(tiles * 4);
    l.tile_base = c.take(tiles * 4);
    l.stat_part = c.take(tiles * 8);
    l.stat_mean = c.take(8);
    for (int k = 0; k < n; k++)
        for (size_t b = 0; b < buffers; b++) l.field[b][k] = c.take(B * row_bytes[k]);
    const size_t scalar_bytes[MB_S_COUNT] = {B * 12, B * 4, B, B * 4, B * 4, B * 4, B * 4 * IMGENV_MB_MAX_SCALARS};
    for (int q = 0; q < MB_S_COUNT; q++)
        for (size_t b = 0; b < buffers; b++) l.scalar[b][q] = c.take(scalar_bytes[q]);
    l.total = c.total;
    return l;
}

// imgenv_rollout_seq_enable (sequences.h): the flags, the index and its tile scratch, then per gathered field and per scalar array
// its `buffers` copies side by side, as the minibatches'.  S = C_max RL sequences, a buffer holds length x batch steps.
enum { SEQ_S_ACTIONS, SEQ_S_REWARDS, SEQ_S_DONES, SEQ_S_DONES_INFO, SEQ_S_INDEX, SEQ_S_WEIGHT, SEQ_S_FIRST, SEQ_S_SCALARS, SEQ_S_SEQ, SEQ_S_SEQ_LEN,
       SEQ_S_STATE0, SEQ_S_STATE1, SEQ_S_COUNT };
struct SeqLayout {
    size_t flag, valid, order, valid_n, tile_count, tile_base;
    size_t field[IMGENV_MB_MAX_BUFFERS][ROLLOUT_TABLE_FIELDS], scalar[IMGENV_MB_MAX_BUFFERS][SEQ_S_COUNT], total;
};
inline SeqLayout plan_seq_layout(const size_t* row_bytes, int n, size_t RL, size_t T, size_t length, size_t batch, size_t buffers, const size_t* state_bytes) {
    SeqLayout l = {};
    const size_t S = plan_seq_chunks(T, length) * RL, tiles = plan_mb_tiles(S), N = length * batch;
    Carve c;
    l.flag = c.take(S);
    l.valid = c.take(S * 4);
    l.order = c.take(S * 4);
    l.valid_n = c.take(4);
    l.tile_count = c.take(tiles * 4);
    l.tile_base = c.take(tiles * 4);
    for (int k = 0; k < n; k++)
        for (size_t b = 0; b < buffers; b++) l.field[b][k] = c.take(N * row_bytes[k]);
    const size_t scalar_bytes[SEQ_S_COUNT] = {N * 12, N * 4, N, N * 4, N * 4, N * 4, N, N * 4 * IMGENV_MB_MAX_SCALARS, batch * 4, batch * 4,
                                              batch * state_bytes[0], batch * state_bytes[1]};
    for (int q = 0; q < SEQ_S_COUNT; q++)
        for (size_t b = 0; b < buffers; b++) l.scalar[b][q] = c.take(scalar_bytes[q]);
    l.total = c.total;
    return l;
}

// imgenv_normalise_enable (normalise.h): D = state_dim, K = the depth of the normalised state stack (0: none), obs / rew = the
// cfg's IMGENV_NORM_OBS / IMGENV_NORM_REWARD.  An array the flags leave out has no bytes.
#define NORM_STATS_WORDS(D) (4 + 2 * (size_t)(D))
struct NormaliseLayout {
    size_t stats, returns, part, part_n, norm_vector_states, norm_state_stack, norm_rewards, total;
};
inline NormaliseLayout plan_normalise_layout(size_t RL, int D, int K, bool obs, bool rew) {
    NormaliseLayout l = {};
    // (the columns of a step's launch -- the observed states and the return -- and of a reset chain's)
    const int cols_step = std::max(1, (obs ? D : 0) + (rew ? 1 : 0)), cols_reset = std::max(1, obs ? D : 0);
    const size_t tiles = std::max(plan_norm_tiles(RL, cols_step), plan_norm_tiles(RL, cols_reset));
    Carve c;
    l.stats = c.take(2 * NORM_STATS_WORDS(D) * 8);
    l.returns = c.take(rew ? 2 * RL * 8 : 0);
    l.part = c.take(tiles * (size_t)cols_step * 16);
    l.part_n = c.take(tiles * 4);
    l.norm_vector_states = c.take(obs ? RL * D * 4 : 0);
    l.norm_state_stack = c.take((size_t)K * RL * D * 4);
    l.norm_rewards = c.take(rew ? RL * 8 : 0);
    l.total = c.total;
    return l;
}

// imgenv_policy_enable (policy.h): a categorical head (`cat`) keeps the index drawn, a Gaussian one the raw sample of its `cols`
// columns (cat: 1); T > 0 (IMGENV_POLICY_STORE, the rollout's horizon) adds what the window stores per slot
struct PolicyLayout {
    size_t index, raw, logp, entropy, pol_raw, pol_logp, pol_value, total;
};
inline PolicyLayout plan_policy_layout(bool cat, size_t cols, size_t RL, size_t T) {
    PolicyLayout l = {};
    Carve c;
    l.index = c.take(cat ? RL * 4 : 0);
    l.raw = c.take(cat ? 0 : RL * cols * 4);
    l.logp = c.take(RL * 4);
    l.entropy = c.take(RL * 4);
    l.pol_raw = c.take(cols * T * RL * 4);
    l.pol_logp = c.take(T * RL * 4);
    l.pol_value = c.take(T > 0 ? (T + 1) * RL * 4 : 0);
    l.total = c.total;
    return l;
}

// imgenv_policy_loss_enable (policy_loss.h): B = max_rows, n = A (cat) or C, n_rec = the workgroups of the largest row launch
// (plan_policy_loss_launch(max_rows, ...).grid), each of which leaves one record of `rec_doubles` (PLOSS_REC) float64
struct PolicyLossLayout {
    size_t logp, entropy, ratio, pg, vl, d_params, d_log_std, d_log_std_shared, d_values, stats, n_bad, inv_w;
    size_t row_m, row_log_s, row_gu, row_w, rec, total;
};
inline PolicyLossLayout plan_policy_loss_layout(bool cat, size_t B, size_t n, size_t n_rec, size_t rec_doubles) {
    PolicyLossLayout l = {};
    Carve c;
    l.logp = c.take(B * 4);
    l.entropy = c.take(B * 4);
    l.ratio = c.take(B * 4);
    l.pg = c.take(B * 4);
    l.vl = c.take(B * 4);
    l.d_params = c.take(B * n * 4);
    l.d_log_std = c.take(cat ? 0 : B * n * 4);
    l.d_log_std_shared = c.take(cat ? 0 : n * 4);
    l.d_values = c.take(B * 4);
    l.stats = c.take(8 * 4);
    l.n_bad = c.take(4);
    l.inv_w = c.take(4);
    l.row_m = c.take(cat ? B * 4 : 0);
    l.row_log_s = c.take(cat ? B * 4 : 0);
    l.row_gu = c.take(B * 4);
    l.row_w = c.take(B * 4);
    l.rec = c.take(n_rec * rec_doubles * 8);
    l.total = c.total;
    return l;
}

// ---------------------------------------------------------------------------------------- in front of the chain: k_actions
// imgenv_actions_decode (actions.h): one lane per local robot, every wavefront whole (the ballot that counts bad rows runs on all
// 64 lanes), no cap and no stride: 2^19 robots are 2048 blocks
inline LaunchShape plan_actions_launch(const PlanHandle& h) { return {(unsigned)((h.RL + ACT_BLOCK - 1) / ACT_BLOCK), ACT_BLOCK, 0}; }
// imgenv_policy_sample (policy.h).  Categorical over A logits: a group of G lanes per local robot, the smallest of 1, 4, 16, 64 that
// leaves a lane at most POL_REG logits (which it then keeps in registers); from A = 1025 on G stays 64 and the lanes re-read
// their ceil(A / 64) logits.  A group never straddles a wavefront (G divides 64) and every wavefront is whole.  Gaussian and the
// values-only call: one lane per robot (n_logits 0).
inline constexpr int plan_policy_group(int n_logits) { return n_logits <= POL_REG ? 1 : n_logits <= 4 * POL_REG ? 4 : n_logits <= 16 * POL_REG ? 16 : 64; }
inline constexpr int plan_policy_per_lane(int n_logits) { return (n_logits + plan_policy_group(n_logits) - 1) / plan_policy_group(n_logits); }
inline LaunchShape plan_policy_launch(const PlanHandle& h, int n_logits) {
    const size_t lanes = (size_t)h.RL * (size_t)plan_policy_group(n_logits);
    return {(unsigned)((lanes + POL_BLOCK - 1) / POL_BLOCK), POL_BLOCK, 0};
}
// imgenv_policy_loss (policy_loss.h): the same groups over the B rows of a minibatch instead of the handle's robots, for the row
// launch and the gradient launch alike (Gaussian: n_logits 0); the row launch leaves one record per workgroup, which is what
// k_ploss_fold's single wavefront folds
inline LaunchShape plan_policy_loss_launch(int rows, int n_logits) {
    const size_t lanes = (size_t)rows * (size_t)plan_policy_group(n_logits);
    return {(unsigned)((lanes + POL_BLOCK - 1) / POL_BLOCK), POL_BLOCK, 0};
}

// ---------------------------------------------------------------------------------------- resets
// Device half of a host-side reset, for every world or the n worlds listed: one upload launch (segment copies | map restore |
// robot state | pedestrian state), the obstacle maps, then view_agent + get_states (img_env.cpp:285-286) for those worlds' robots.
struct ResetPlan {
    int per_seg = 1;  // workgroups per staged segment
    LaunchShape apply, obstacles, bbox;
};
inline ResetPlan plan_reset(const PlanHandle& h, const PlanChain& c, size_t n_seg, size_t seg_max, size_t n_inst) {
    ResetPlan r;
    r.per_seg = (int)std::min<size_t>((seg_max / 16 + 255) / 256 + 1, 16);
    r.apply = {(unsigned)(n_seg * r.per_seg + (size_t)c.act_nw * MAP_BLOCKS + (c.act_ng + 255) / 256 + (c.act_np + 255) / 256), 256, 0};
    r.obstacles = {(unsigned)n_inst, 256, 0};  // one workgroup per obstacle
    r.bbox = {(unsigned)((h.RL + 255) / 256), 256, 0};
    return r;
}
// Device-side reset chain: nobody on the host knows how many worlds the step finished, so the grids are sized for a guess (four
// times the last count the host has seen; the kernels stride over the rest if there are more) ...
struct DevResetPlan {
    int guess = 0, restore_blocks = 4 * MAP_BLOCKS /* per world */, parts = 4 /* workgroups per obstacle */;
    LaunchShape restore, obstacles;
};
inline DevResetPlan plan_dev_reset(const PlanHandle& h, int last_n, int n_obstacles) {
    DevResetPlan r;
    r.guess = std::min(h.W, std::max(16, 4 * std::max(last_n, 0)));
    r.restore = {(unsigned)(r.guess * r.restore_blocks), 256, 0};
    r.obstacles = {(unsigned)(r.guess * n_obstacles * r.parts), 256, 0};
    return r;
}
// k_tracks_install (track_bank.h): a workgroup per world that takes its recorded crowd from the bank.  A host chain knows its
// worlds (n_worlds of them; none: nothing to launch, grid 0); the device chain sizes the grid for plan_dev_reset's guess and the
// workgroups stride over the count the device holds.  A world's copy is `words` 8-byte words for each of the two tables
// (Pw * cap * 3: an odd product leaves every other world's rows 8-byte aligned only, so the unit of the copy is never wider)
// in `rounds` rounds of the workgroup's lanes.
struct TracksPlan {
    LaunchShape install;
    size_t words = 0;
    int rounds = 0;
};
inline TracksPlan plan_tracks_install(const PlanHandle& h, int n_worlds, bool n_dev, int last_n, int cap) {
    TracksPlan t;
    const int grid = n_dev ? plan_dev_reset(h, last_n, 0).guess : std::max(n_worlds, 0);
    t.install = {(unsigned)grid, TRACKS_BLOCK, 0};
    t.words = (size_t)h.Pw * (size_t)std::max(cap, 0) * 3;
    t.rounds = (int)((t.words + TRACKS_BLOCK - 1) / TRACKS_BLOCK);
    return t;
}
// ... and the variants of the chain behind chosen by the robots it is expected to cover (twice the last count: with four times,
// 64 worlds of 4 pedestrians sat ON the 1024 threshold and flipped between the kernel variants)
inline int plan_act_hint(const PlanHandle& h, int last_n) { return std::max(8, 2 * std::max(last_n, 0)) * std::max(std::max(h.Rw, h.Pw), 1); }
