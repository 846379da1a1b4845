// imgenv_hip.hip -- C ABI (include/imgenv.h) of the MI355X-native img_env step() path.
// Host orchestration of ImgEnv::_init/_reset/_step (img_env.cpp:83-160, 162-292, 421-525) as a fixed
// sequence of HIP kernels on one stream; all simulator state lives in HBM for the life of the handle.
//
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -ffp-contract=off (see __graft_entry__.py)
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <rccl/rccl.h>
#include <stdio.h>

#include <string>
#include <chrono>
#include <memory>
#include <unordered_map>
#include <vector>

#define WAVE_SZ 64
#include "../../include/imgenv.h"
#include "host_tables.h"
#include "cv_resize.h"
#include "spawn_host.h"
#include "launch_plan.h"
#include "out_fields.h"
#include "create_plan.h"
#include "reset_plan.h"
#include "obs_fields.h"
#include "kernels.h"
#include "world.h"
#include "stack.h"
#include "episodes.h"
#include "episode_log.h"
#include "actions.h"
#include "policy.h"
#include "policy_loss.h"
#include "obs_post.h"
#include "final_obs.h"
#include "rollout.h"
#include "minibatch.h"
#include "sequences.h"
#include "ped_draw.h"
#include "map_bank.h"
#include "spawn_slot.h"
#include "bank_host.h"
#include "normalise.h"
#include "feature_plan.h"

static_assert(OBS_POST_PLAN_DIM == OBS_POST_DIM, "feature_plan.h against obs_post.h");

static thread_local char g_err[512] = "";
#define FAIL(code, ...)                              \
    do {                                             \
        snprintf(g_err, sizeof(g_err), __VA_ARGS__); \
        return (code);                               \
    } while (0)
#define HIPCHK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) FAIL(IMGENV_EDEVICE, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// What the handle keeps of one optional feature (struct imgenv below has one record per feature, some with cursors of their own).
// Per member: who sets it / who clears it / what it means while set.
struct NoCfg {};  // (a feature whose repeated call is judged without a stored cfg)
template <typename Dev, typename Cfg, typename Out>
struct Feature {
    bool on = false;  // enable_done / never / imgenv_X_enable has succeeded: dev, cfg and out are valid
    Dev dev = {};     // imgenv_X_enable, just before enable_done / never / the kernel arguments the launches copy and complete
    Cfg cfg = {};     // likewise / never / the cfg of the first call: what a repeated call is compared against
    Out out = {};     // enable_done / never (a later enable may add a normalised field's pointer to norm.out) / what imgenv_X_outputs and a repeated enable hand back
};

struct imgenv {
    imgenv_cfg cfg;
    ViewGeom geom;
    int R = 0, P = 0, r0 = 0, r1 = 0, RL = 0, NA = 0, Hg = 0, Wg = 0, PP = 2;
    int W = 1, Rw = 0, Pw = 0;  // independent worlds in this handle, robots / pedestrians per world
    size_t Gs = 0;              // cells between two worlds' copies of a grid layer
    std::vector<int> world_epoch;  // h->elapsed at each world's last reset
    std::vector<char> world_ready;
    int* d_world_epoch = nullptr;
    int* d_wobst = nullptr;        // [4][W]: obstacle base, node base, #obstacles, root per world
    std::vector<int> wobst;
    std::vector<RobotClassHost> rcls;
    std::vector<PedClassHost> pcls;
    std::vector<int> robot_cls, ped_cls;
    std::vector<uint8_t> static_map;
    std::vector<double> rsl;
    std::vector<float> pmax;
    DevWorld d;
    PlanHandle plan;  // what the launch rules (launch_plan.h) read of this handle: plan_facts
    int raster_pack = -1;  // IMGENV_RASTER_PACK when the handle was created (measurement switch; -1: unset, the plan's rule)
    int obs_room = -1;     // IMGENV_OBS_ROOM when the handle was created (measurement switch, plan_obs_lds; -1: unset, the plan's rule)
    std::vector<void*> allocs;
    unsigned char* arena = nullptr;
    bool own_arena = false;
    imgenv_out out;
    uint8_t* d_obs_map = nullptr;
    RvoObstDev* d_obst = nullptr;
    RvoNodeDev* d_nodes = nullptr;
    int cap_obst = 0, cap_nodes = 0;
    double* d_traj = nullptr;
    double* d_traj_v = nullptr;  // dataset scene
    // IMGENV_TRACE_RESET: where the host's time goes inside a reset entry point, by phase, reported every 200 calls of this handle
    struct ResetTrace {
        double acc[4] = {0, 0, 0, 0};
        long calls = 0, worlds = 0;
        static bool on() {
            static const bool set = getenv("IMGENV_TRACE_RESET") != nullptr;
            return set;
        }
        static double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
        bool add(const double* us, int phases, int n_worlds) {  // a call's microseconds by phase; true: time to report
            for (int q = 0; q < phases; q++) acc[q] += us[q];
            worlds += n_worlds;
            return ++calls % 200 == 0;
        }
    };
    // The host-side reset in flight (reset_all / reset_worlds: prepare, refuse, commit -- DESIGN.md §8; its device-free half is
    // reset_plan.h).  Everything a reset uploads goes through page-locked chunks and reaches the device in ONE launch; nothing here
    // means anything between two resets except the chunks, the vectors' capacity and the trace.  Per member: who sets it / who
    // clears it / what it means while set.
    struct Chunk { unsigned char* p; size_t cap, used; };
    // STAGE_GENS generations of chunks, used round-robin: a reset only ever waits for the reset STAGE_GENS calls back (the
    // host may run several steps ahead of the device; waiting for the previous reset would drain that queue every time)
    static constexpr int STAGE_GENS = 4;
    struct ResetStage {
        std::vector<ResetWorld> worlds;  // reset_prepare / the next reset_prepare / what each listed world's batch brings, in list order; commit swaps the RVO sets out
        std::vector<Chunk> chunks[STAGE_GENS];  // stage_room adds one / imgenv_destroy / page-locked memory of generation g; stage_begin empties the one it takes
        hipEvent_t ev_gen[STAGE_GENS] = {nullptr, nullptr, nullptr, nullptr};  // stage_begin creates, stage_end records / imgenv_destroy / behind the launches that read generation g
        bool gen_pending[STAGE_GENS] = {false, false, false, false};  // stage_end / stage_begin, having waited for ev_gen[g] / the device may still read generation g
        int gen = 0;                  // stage_begin advances / never / the generation this reset stages into
        std::vector<StageSeg> segs;   // stage_seg / stage_begin, reset_apply behind its launch / the copies k_reset_apply makes
        size_t seg_max = 0;           // stage_seg / with segs / the largest of them (ResetPlan::per_seg)
        double *rob3 = nullptr, *ped3 = nullptr;  // reset_blocks / never (they point into this generation) / robot and pedestrian rows in list order, read by k_reset_apply
        ResetRobot* rr = nullptr;     // likewise: goals of the local robots
        int* list = nullptr;          // likewise: the listed worlds (nullptr: every world)
        std::vector<int> fed, fed_ids;  // stage_world_peds / reset_blocks, reset_tracks behind its launch / the bank-fed worlds of this reset and the host's draw for each (-1: the device resolves)
        ObstInst* d_inst = nullptr;   // reset_obstacles grows it / never / device room for the obstacle instances of one reset
        size_t cap_inst = 0;
        ResetTrace trace;             // reset_worlds / never
    } rs;
    uint8_t* d_static_map = nullptr;  // the map every reset starts from; with a bank (imgenv_maps_add) [n_maps][map_stride], map 0 first
    // map bank (include/imgenv.h: imgenv_maps_add; csrc/map_bank.h)
    int Hg_in = 0, Wg_in = 0;       // the size of the map as imgenv_create received it (before the load-time resize)
    int n_maps = 1;
    size_t map_stride = 0;          // bytes between two maps of the bank
    int* d_map_cur = nullptr;       // [W] map of each world's current episode (nullptr: no bank)
    int* d_map_next = nullptr;      // [W] map each world's next reset starts from
    int maps_policy = 0;            // IMGENV_MAPS_*
    // track bank (include/imgenv.h: imgenv_tracks_add; csrc/track_bank.h)
    int n_track_sets = 0, trk_cap = 0;   // sets of the bank (0: none); records per pedestrian in it
    double *d_trk_traj = nullptr, *d_trk_traj_v = nullptr, *d_trk_pose3 = nullptr;
    int* d_trk_len = nullptr;
    int *d_trk_cur = nullptr, *d_trk_next = nullptr;  // [W] (nullptr: no bank)
    uint32_t* d_trk_count = nullptr;                  // [W]
    int tracks_policy = 0, tracks_repeat = 1;         // IMGENV_TRACKS_*
    // scenario bank (include/imgenv.h: imgenv_scenarios_add; csrc/scenario_bank.h)
    int n_scn = 0, scn_obst = 0;               // episodes of the bank (0: none); obstacles of each
    std::vector<SlotAgent> scn_agents;         // [n_scn][Rw + Pw] the host copy (imgenv_reset_worlds_scenarios, checkers)
    std::vector<SlotObstacle> scn_obstacles;   // [n_scn][scn_obst]
    SlotAgent* d_scn_agents = nullptr;
    SlotObstacle* d_scn_obst = nullptr;
    int scn_policy = 0;                        // IMGENV_SCENARIOS_*
    uint64_t scn_first = 0;
    int* d_scn_world = nullptr;                // [W] the scenario of each world's last HOST reset, -1: not from the bank
    unsigned long long* d_scn_mark = nullptr;  // [W] the placement number the world held at that reset (k_scenario_mark)
    // which policy the device's placements were filled under: epoch e covers the placement numbers from its start on, the start
    // being the device's count when imgenv_scenarios_policy was queued -- copied on the device, read at imgenv_world_scenarios
    struct ScnEpoch { int policy; uint64_t first; };
    std::vector<ScnEpoch> scn_epochs;
    unsigned long long* d_scn_starts = nullptr;  // [scn_starts_cap]
    size_t scn_starts_cap = 0;
    int* d_act_list = nullptr;
    bool big_view = false;   // the view is beyond k_view's packing, or shrunk by cv2.resize: the kernels of view_big.h
    int big_tap_chunks_dyn = 0;  // k_taps_big workgroups per robot in a step (the largest list of any class: BigClassDev::tap_chunks)
    size_t lds_view_big = 0;
    bool big_bits_in_lds = true;  // the crop bitmap of one robot fits the LDS next to the hit words
    int big_max_crop = 1, big_full_chunks = 1;
    // early-observation steps (world.h): k_obs is launched with the step, beside the move (k_move_raster), from snapshots
    bool early = false;             // the handle can run them (IMGENV_EARLY_OBS=0 in the environment switches them off)
    float4* ped_snap[2] = {nullptr, nullptr};  // behind k_orca: launch q over every world writes ped_snap[q & 1] (plan_snap_turn)
    double* rec_snap[2] = {nullptr, nullptr};  // behind k_view, likewise
    // What a step hands from imgenv_step_begin to the end of its chain, and a chain to the next one.  What launch_views and
    // imgenv_step_begin do with it is decided in launch_plan.h ("ordering"; DESIGN.md §4 has the side wiring as a table); an
    // abandoned step is recovered by step_recover alone.  Per member: who sets it / who clears it / what it means while set.
    struct StepState {
        bool in_step = false;      // imgenv_step_flags, around its imgenv_step_begin / the same / begin and end are one call: the move may be left to the chain
        const float* actions = nullptr;  // step_entry / never (the caller keeps them until the chain's end) / the step's actions: a fused move and the tails read them
        bool move_pending = false; // imgenv_step_begin (StepPlan::fuse_move) / launch_views / the chain's raster launch does the move (k_move_raster)
        bool fork_on_move = false; // step_move (StepPlan::fork_on_move) / launch_obs, early_obs / ev_fork went out on k_integrate's packet: not recorded again
        bool obs_forked = false;   // launch_obs, early_obs / launch_side, step_recover / the step's k_obs is in flight on its stream
        bool early = false;        // early_obs / launch_views / that k_obs went out in front of the move: a solve on its stream waits for ev_fork
        bool chain_open = false;   // chain_begin, early_obs / launch_views' end / tail_sig, tail_cnt may hold bits: the next chain_begin clears them first
        uint32_t gate_seq = 0;     // imgenv_step_begin counts the early steps / never / the number k_integrate opens the gate with and k_gate waits for (world.h: sync)
        unsigned orca_seq = 0;     // launch_side counts k_orca over every world / never / ped_snap's turn; 0: no snapshot yet
        unsigned view_seq = 0;     // launch_compose_views counts k_view over every world / never / rec_snap's turn
        bool obs_exists = false;   // launch_views' end / never / a chain has completed on this handle: its output rows hold an observation (the features only read it)
        uint64_t chain_seq = 0;    // launch_views and imgenv_rollout_begin count / never / chains and rollout windows queued so far: a minibatch index is of one value
    } step;
    // The social-force crowd a step AHEAD (sfm.h: SfmDev *_out): crowds that ignore the robots (relation_ped_robo = 0) depend on
    // nothing of a step, so k_sfm for step t + 1 runs on a stream of its own underneath step t's rasters and views, reads the
    // crowd as it is and leaves the next state in a second set of arrays; step t + 1 swaps the sets and only publishes
    // (k_sfm_publish).  A reset in between drops what was computed ahead.  plan_crowd_step decides, step_crowd executes.
    struct CrowdAhead {
        bool can = false;          // create_facts (CreatePlan::sfm_ahead) / imgenv_step_autoreset_device, for good: its kernels reset crowds unseen / the handle does that
        bool valid = false;        // sfm_launch_ahead / sfm_ahead_drop / `other` holds the next step's state (computed or being computed on `stream`)
        int steps_since_reset = 0; // step_crowd counts / sfm_ahead_drop / 0: the next step launches nothing ahead
        int par = 0;               // step_crowd flips / never / which ev_in the next step leaves
        int wait = -1;             // step_crowd / sfm_launch_ahead / >= 0: this imgenv_step_begin still owes the launch ahead, behind ev_in[wait]
        SfmDev other;              // the other set of the arrays a step writes (sfm_swap_sets)
        hipStream_t stream = nullptr;
        hipEvent_t ev = nullptr;   // behind the launch ahead
        hipEvent_t ev_in[2] = {nullptr, nullptr};  // behind a step's last access to the crowd's sets on the caller's stream, by step parity
    } crowd;
    bool gates_work = false;     // k_gate_probe's verdict: kernels of two streams run side by side in this process
    bool sum = false;        // SUM mode of the class layer (world.h): base class + counts kept by the agents themselves, no k_compose
    bool stamp = false;      // STAMP mode of the class layer (world.h) instead of two owner layers + k_compose
    uint32_t stamp_seq = 0;  // steps so far: the stamps of a step carry tag stamp_seq % STAMP_TAGS + 1
    int* d_traj_len = nullptr;
    int traj_cap = 0;
    int elapsed = 0;
    bool has_reset = false;
    int launches = 0;
    size_t lds_view = 0, lds_obs = 0;
    int obs_E = 0;  // sort slots per lane of k_obs (0: LDS sort)
    int n_sub = 0;  // 0.05 s sub-steps of Agent::cmd per step (agent.cpp:221-236)
    bool pow2 = false;
    // the ORCA solve of step t+1 only needs what exists after the rasters of step t, so it runs on a side
    // stream underneath the view / observation kernels of step t (200 waves alone cannot fill the chip)
    ncclComm_t comm = nullptr;  // optional: native RCCL exchange inside imgenv_step
    int comm_ranks = 0;
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipStream_t side2 = nullptr;  // pedestrian observation (k_obs) underneath raster / compose / view
    hipEvent_t ev_fork2 = nullptr, ev_join2 = nullptr;
    bool serial = false;  // IMGENV_SERIAL=1: no side streams (profiling aid)
    volatile int* err_host = nullptr;  // [8] page-locked flags the kernels raise on overflow; checked at every API call
    volatile int* finished_host = nullptr;  // [1 + W] page-locked: the worlds whose robots are all done (k_finished)
    // imgenv_step_autoreset draws the placements of the next few seeds while the device is still busy with the step
    std::unordered_map<uint64_t, std::unique_ptr<SpawnOut>> spawn_ahead;
    uint64_t spawn_ahead_cfg = 0;  // fingerprint of the spawn cfg the placements were drawn from
    int spawn_ahead_n = 8;
    ResetTrace trace_autoreset;  // imgenv_step_autoreset / never
    // Device-side auto-reset (csrc/spawn_device.h): a pool of placements drawn ahead on a side stream.  Per member: who sets it /
    // who clears it / what it means while set.
    struct DevReset {
        bool ready = false;         // spawn_device_setup / the same, while another spawn cfg rebuilds the pool / `pool` is built and its first fill queued
        bool used = false;          // imgenv_step_autoreset_device / reset_all / kernels have reset worlds: h->rvos and the host's wobst no longer say what the device holds
        int fill_due = 0;           // autoreset_device_chain (SPAWN_FILL_PERIOD), counting down / set-up, refresh, imgenv_scenarios_policy: 0 / calls until the pool is refilled
        bool fill_pending = false;  // launch_pool_fill / autoreset_device_chain, having made the stream wait / ev_fill is behind a fill nothing has waited for yet
        int act_hint = 0;           // imgenv_step_autoreset_device / never / robots the reset chain is expected to cover (picks the small-launch kernel variants)
        uint64_t fp = 0;            // imgenv_step_autoreset_device / never / fingerprint of the spawn cfg the pool was built from
        hipStream_t side3 = nullptr;  // spawn_device_setup / imgenv_destroy / the fills' stream
        hipEvent_t ev_fill = nullptr, ev_consumed = nullptr;  // likewise / behind a fill; behind the chain that consumed placements
        SpawnDev pool = {};         // spawn_device_setup builds, spawn_dev_refresh re-aims / never / what every kernel of the chain gets by value (valid while ready)
    } dev;
    // (The chain as a replayed hipGraph was measured in round 4 and dropped in round 6: this runtime issues a replayed graph node
    // by node, 222 us of host time per step against 195 us for the same ~25 plain launches -- docs/HISTORY.md.)
    // output guards (include/imgenv.h: IMGENV_FLAG_CHECK_OUTPUTS / IMGENV_FLAG_FULL_REWRITE)
    unsigned char* pub_arena = nullptr;  // FULL_REWRITE: what imgenv_outputs hands out -- a copy of the working arena made at the end of every chain
    bool own_pub = false;
    size_t arena_bytes = 0;
    imgenv_out pub_out;
    bool guard_check = false, guard_sealed = false;
    int guard_left = -1;  // IMGENV_FLAG_CHECK_OUTPUTS_FIRST: verifications until the guard switches itself off (-1: never)
    OutSpan* d_spans = nullptr;          // CHECK_OUTPUTS: the output arrays as (pointer, bytes, first block) ...
    int n_spans = 0, span_blocks = 0;
    unsigned long long* d_sums = nullptr;  // ... and their checksums: [2][n_spans], sealed | found at the next call
    const char* span_name[40];
    // The optional features (include/imgenv.h: imgenv_*_enable): one record each -- Feature's four members and the
    // feature's own host cursors.  What an enable call decides before it touches the device is feature_plan.h's, from
    // feature_facts(h).  Per member: who sets it / who clears it / what it means while set.
    // observation stacks (csrc/stack.h); dev.n_fields == 0: every depth is 0 or 1, nothing to launch
    Feature<StackDev, NoCfg, imgenv_stack_out> stack;
    // episode statistics (csrc/episodes.h)
    struct Episodes : Feature<EpisodesDev, imgenv_episodes_cfg, imgenv_episodes_out> {
        size_t clear_bytes = 0;      // imgenv_episodes_enable / never / what imgenv_episodes_clear zeroes, from dev.f on
    } ep;
    // episode log (csrc/episode_log.h); its capacity is dev's
    Feature<EpisodeLogDev, NoCfg, imgenv_episode_log_out> eplog;
    // action decoding (csrc/actions.h)
    struct Actions : Feature<ActionsDev, imgenv_actions_cfg, imgenv_actions_out> {
        std::vector<float> table;    // imgenv_actions_enable / never / the rows of a TABLE cfg: cfg.table is null, a repeated call is compared against this copy
        int decode_launches = 0;     // imgenv_actions_decode, imgenv_policy_sample count / step_entry / k_actions and k_policy launches since the last step: they count with the step that consumes them
    } act;
    // the policy head (csrc/policy.h); dev is what every launch shares: params, draw, flags and the slot's pointers are the call's
    Feature<PolicyDev, imgenv_policy_cfg, imgenv_policy_out> pol;
    // PPO's loss (csrc/policy_loss.h); dev is the handle's arrays: inputs, coefficients and rows are the call's
    Feature<PlossDev, imgenv_policy_loss_cfg, imgenv_policy_loss_out> ploss;
    // observation post-processing (csrc/obs_post.h)
    Feature<ObsPostDev, imgenv_obs_post_cfg, imgenv_obs_post_out> post;
    // final observations (csrc/final_obs.h)
    Feature<FinalObsDev, imgenv_final_obs_cfg, imgenv_final_obs_out> final_obs;
    // rollout storage (csrc/rollout.h)
    struct Rollout : Feature<RolloutDev, imgenv_rollout_cfg, imgenv_rollout_out> {
        bool begun = false;          // imgenv_rollout_begin / imgenv_rollout_enable / a window is open: chains store
        int n = 0;                   // tail_rollout counts the step chains / imgenv_rollout_begin / the cursor: transitions stored in this window
        uint32_t turn = 0;           // tail_rollout counts the reset chains / imgenv_rollout_begin / reset chains stored in this window
        size_t row_bytes[ROLLOUT_TABLE_FIELDS];  // imgenv_rollout_enable / never / the row of entry k of dev.f ...
        int field_id[ROLLOUT_TABLE_FIELDS];      // ... and which field (obs_fields.h) it is
    } roll;
    // rollout minibatches (csrc/minibatch.h); dev holds the field table and the ring's scalars, its dst pointers are the call's buffer's
    struct Minibatch : Feature<MbGatherDev, imgenv_minibatch_cfg, imgenv_minibatch_out> {
        bool indexed = false;        // imgenv_rollout_index / imgenv_rollout_minibatch_enable / the valid list exists, of the generation (gen_n, gen_seq)
        int gen_n = 0;               // imgenv_rollout_index / never / roll.n when the index was made
        uint64_t gen_seq = 0;        // imgenv_rollout_index / never / step.chain_seq then: any chain or window since makes the index stale
        bool shuffled = false;       // imgenv_rollout_shuffle / imgenv_rollout_index / `order` is a permutation of that index
        unsigned char* dst[IMGENV_MB_MAX_BUFFERS][ROLLOUT_TABLE_FIELDS];  // imgenv_rollout_minibatch_enable / never / where buffer b keeps entry k of dev.f, the normalised fields included
        PedDrawDev draw = {};        // imgenv_rollout_minibatch_enable / never / IMGENV_ROLLOUT_PED_MAPS_DRAWN is selected (draw.vec != nullptr): k_ped_draw's arguments but for the call's buffer and minibatch
        float* draw_dst[IMGENV_MB_MAX_BUFFERS] = {};  // imgenv_rollout_minibatch_enable / never / buffer b's mb_ped_maps where they are drawn
    } mb;
    // sequence minibatches (csrc/sequences.h); dev holds the field table, the ring's scalars and the sizes, its dst pointers are the call's buffer's
    struct Sequences : Feature<SeqGatherDev, imgenv_seq_cfg, imgenv_seq_out> {
        bool indexed = false;        // imgenv_rollout_seq_index / imgenv_rollout_seq_enable / seq_valid exists, of the generation (gen_n, gen_seq)
        int gen_n = 0;               // imgenv_rollout_seq_index / never / roll.n when the index was made
        uint64_t gen_seq = 0;        // imgenv_rollout_seq_index / never / step.chain_seq then
        bool shuffled = false;       // imgenv_rollout_seq_shuffle / imgenv_rollout_seq_index / seq_order is a permutation of that index
        unsigned char* dst[IMGENV_MB_MAX_BUFFERS][ROLLOUT_TABLE_FIELDS];  // imgenv_rollout_seq_enable / never / where buffer b keeps entry k of dev.f
        PedDrawDev draw = {};        // imgenv_rollout_seq_enable / never / IMGENV_ROLLOUT_PED_MAPS_DRAWN is selected (draw.vec != nullptr): k_ped_draw's arguments but for the call's buffer
        float* draw_dst[IMGENV_MB_MAX_BUFFERS] = {};  // imgenv_rollout_seq_enable / never / buffer b's mb_ped_maps where they are drawn
    } seq;
    // running normalisation (csrc/normalise.h); dev.n_obs as enabled: n_ret, cols, update, the turns and the rows are the launch's
    struct Normalise : Feature<NormDev, imgenv_normalise_cfg, imgenv_normalise_out> {
        bool training = true;        // imgenv_normalise_enable, imgenv_normalise_training / the latter / the chains update the statistics
        uint32_t turn = 0;           // tail_normalise counts / never / chains that have moved the statistics: which word of dev.stats is read
        uint32_t ret_turn = 0;       // tail_normalise counts / never / step chains that have moved the returns: which word of dev.returns is read
    } norm;
    std::vector<RvoObstacles> rvos;  // one obstacle set per world
    int sfm_cap_obs = 0;
    std::vector<int> sfm_nobs_w;  // pedscene, several worlds: obstacle segments of each world's crowd
    // live timing (imgenv_timing)
    int t_mode = 0, t_which = -1;
    unsigned t_tick = 0;
    std::vector<hipEvent_t> t_ev;
    std::vector<int> t_id;  // kernel id of event pair q
    size_t t_used = 0;
    double t_ms[IMGENV_K_COUNT] = {0};
    int64_t t_cnt[IMGENV_K_COUNT] = {0};
};

// RCCL is resolved at run time so that single-GPU users do not need it: prefer the copy the process already
// loaded (torch ships one), then the ROCm one
struct RcclApi {
    void* lib = nullptr;
    decltype(&ncclGetUniqueId) get_id = nullptr;
    decltype(&ncclCommInitRank) init_rank = nullptr;
    decltype(&ncclAllGather) all_gather = nullptr;
    decltype(&ncclCommDestroy) destroy = nullptr;
    decltype(&ncclGetErrorString) err = nullptr;
    decltype(&ncclCommCount) count = nullptr;
    decltype(&ncclCommUserRank) user_rank = nullptr;
};
static RcclApi* rccl_api() {
    static RcclApi api;
    static bool tried = false;
    if (!tried) {
        tried = true;
        const char* names[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"};
        void* lib = dlopen(names[0], RTLD_NOW | RTLD_NOLOAD);
        for (int q = 0; !lib && q < 3; q++) lib = dlopen(names[q], RTLD_NOW | RTLD_GLOBAL);
        if (lib) {
            api.get_id = (decltype(api.get_id))dlsym(lib, "ncclGetUniqueId");
            api.init_rank = (decltype(api.init_rank))dlsym(lib, "ncclCommInitRank");
            api.all_gather = (decltype(api.all_gather))dlsym(lib, "ncclAllGather");
            api.destroy = (decltype(api.destroy))dlsym(lib, "ncclCommDestroy");
            api.err = (decltype(api.err))dlsym(lib, "ncclGetErrorString");
            api.count = (decltype(api.count))dlsym(lib, "ncclCommCount");
            api.user_rank = (decltype(api.user_rank))dlsym(lib, "ncclCommUserRank");
            if (api.count && api.user_rank && api.get_id && api.init_rank && api.all_gather && api.destroy && api.err) api.lib = lib;
        }
    }
    return api.lib ? &api : nullptr;
}

static const char* const KERNEL_NAMES[IMGENV_K_COUNT] = {"k_orca", "k_ped_update", "k_integrate", "k_raster", "k_compose",
                                                         "k_view", "k_obs", "k_tail", "k_crop_big", "k_fullview_big", "k_taps_big", "k_move_raster", "rccl_all_gather",
                                                         "k_remote"};
extern "C" const char* imgenv_kernel_name(int id) { return (id >= 0 && id < IMGENV_K_COUNT) ? KERNEL_NAMES[id] : ""; }

static int timing_flush(imgenv* h) {
    for (size_t q = 0; q < h->t_used; q++) {
        float ms = 0;
        HIPCHK(hipEventSynchronize(h->t_ev[2 * q + 1]));
        HIPCHK(hipEventElapsedTime(&ms, h->t_ev[2 * q], h->t_ev[2 * q + 1]));
        h->t_ms[h->t_id[q]] += ms;
        h->t_cnt[h->t_id[q]] += 1;
    }
    h->t_used = 0;
    return 0;
}
// mode 1: every launch of every kernel; mode 2: every 8th launch of one kernel (an event pair costs the stream a
// dependency barrier, ~5 us of idle GPU, so the timed bench pass samples instead of bracketing every step)
static inline bool timing_on(imgenv* h, int id) {
    if (h->t_mode == 1) return true;
    return h->t_mode == 2 && h->t_which == id && (h->t_tick++ & 7) == 0;
}
static int timing_mark(imgenv* h, int id, hipStream_t st, int end) {
    if (!end) {
        if (h->t_used * 2 + 2 > h->t_ev.size()) {
            if (h->t_ev.size() >= 16384) {
                if (int rc = timing_flush(h)) return rc;
            } else {
                for (int q = 0; q < 2; q++) {
                    hipEvent_t e;
                    HIPCHK(hipEventCreate(&e));
                    h->t_ev.push_back(e);
                }
                h->t_id.push_back(id);
            }
        }
        h->t_id[h->t_used] = id;
        HIPCHK(hipEventRecord(h->t_ev[2 * h->t_used], st));
    } else {
        HIPCHK(hipEventRecord(h->t_ev[2 * h->t_used + 1], st));
        h->t_used++;
    }
    return 0;
}
// launch wrapper: optional event pair on the launch stream around one kernel
#define TIMED(h, id, st, launch)                                       \
    do {                                                               \
        const bool on_ = timing_on(h, id);                             \
        if (on_) { if (int rc_ = timing_mark(h, id, st, 0)) return rc_; } \
        launch;                                                        \
        if (on_) { if (int rc_ = timing_mark(h, id, st, 1)) return rc_; } \
    } while (0)

extern "C" int imgenv_timing(imgenv_t* h, int mode, int which) {
    if (!h || mode < 0 || mode > 2) FAIL(IMGENV_EINVAL, "bad timing mode");
    if (int rc = timing_flush(h)) return rc;
    if (mode != 0) {  // create the event pool up front: hipEventCreate inside a timed region would be measured
        const size_t want = mode == 1 ? 2 * 64 * IMGENV_K_COUNT : 2 * 1024;
        while (h->t_ev.size() < want) {
            hipEvent_t e;
            HIPCHK(hipEventCreate(&e));
            h->t_ev.push_back(e);
            if (h->t_ev.size() % 2 == 0) h->t_id.push_back(0);
        }
    }
    h->t_mode = mode;
    h->t_which = which;
    for (int q = 0; q < IMGENV_K_COUNT; q++) {
        h->t_ms[q] = 0;
        h->t_cnt[q] = 0;
    }
    return IMGENV_OK;
}
extern "C" int imgenv_timing_read(imgenv_t* h, double* total_ms, int64_t* launches) {
    if (!h || !total_ms || !launches) FAIL(IMGENV_EINVAL, "null argument");
    if (int rc = timing_flush(h)) return rc;
    for (int q = 0; q < IMGENV_K_COUNT; q++) {
        total_ms[q] = h->t_ms[q];
        launches[q] = h->t_cnt[q];
    }
    return IMGENV_OK;
}

// "hip-gfx950" is the product build only: a library compiled with any work-skipping experiment switch or with the
// profiling instrumentation says so, so that a number measured on it can never pass for the product's
#if defined(IMGENV_EXP_STOP_AFTER)
extern "C" const char* imgenv_backend(void) { return "hip-gfx950-EXPERIMENT-work-skipped"; }
#elif defined(IMGENV_PHASE_PROFILE) || defined(IMGENV_WAVE_TIMELINE) || defined(IMGENV_EXP_RESOLVE_STATS) || defined(IMGENV_EXP_TINY_RESOLVE) || \
    defined(IMGENV_EXP_SKEW) || defined(IMGENV_EXP_EVERY_CELL)
extern "C" const char* imgenv_backend(void) { return "hip-gfx950-profile-instrumented"; }
#else
extern "C" const char* imgenv_backend(void) { return "hip-gfx950"; }
#endif
// which sources + flags this library was compiled from (__graft_entry__.source_id): counter files under profiles/ name the
// build they were collected on, and bench.py only quotes them for the library it is running
#ifndef IMGENV_BUILD_ID
#define IMGENV_BUILD_ID "unstamped"
#endif
// (the id sits behind a marker so that a build script can read it out of the file's bytes without loading the library into its
// own process: a dlopen'ed image is never replaced by a rebuild of the same path -- __graft_entry__._built_id)
extern "C" const char imgenv_build_marker[] = "IMGENV_BUILD_ID=" IMGENV_BUILD_ID;
extern "C" const char* imgenv_build_id(void) { return imgenv_build_marker + 16; }
extern "C" int32_t imgenv_abi_version(void) { return IMGENV_ABI_VERSION; }
extern "C" const char* imgenv_last_error(void) { return g_err; }

// ---------------------------------------------------------------------------------------- arena
// (the arrays, their order and their sizes: out_fields.h)
extern "C" int64_t imgenv_arena_bytes(const imgenv_cfg* cfg) {
    if (!cfg || cfg->struct_size != (int32_t)sizeof(imgenv_cfg)) return -1;
    int r0, r1;
    if (shard_of(*cfg, r0, r1)) return -1;
    const ViewGeom g = make_view_geom(*cfg);
    return (int64_t)plan_arena(out_facts(*cfg, g.Hv, g.Wv, g.B, r1 - r0)).total;
}

// ---------------------------------------------------------------------------------------- helpers
template <typename T>
static int dev_alloc(imgenv* h, T** out, size_t n, int fill = 0) {
    void* p = nullptr;
    const size_t bytes = sizeof(T) * (n ? n : 1);
    HIPCHK(hipMalloc(&p, bytes));
    h->allocs.push_back(p);
    HIPCHK(hipMemset(p, fill, bytes));
    *out = (T*)p;
    return 0;
}
// hands one dev_alloc'd block back before the handle dies (the caller has made sure nothing in flight uses it)
template <typename T>
static void dev_free(imgenv* h, T*& p) {
    if (!p) return;
    for (size_t q = 0; q < h->allocs.size(); q++)
        if (h->allocs[q] == (void*)p) {
            h->allocs[q] = h->allocs.back();
            h->allocs.pop_back();
            (void)hipFree((void*)p);
            break;
        }
    p = nullptr;
}
template <typename T>
static int dev_upload(imgenv* h, const T** out, const std::vector<T>& v) {
    T* p = nullptr;
    if (int rc = dev_alloc(h, &p, v.size())) return rc;
    if (!v.empty()) HIPCHK(hipMemcpy(p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice));
    *out = p;
    return 0;
}
// DevTxn (bank_host.h) over the device: what imgenv_maps_add, imgenv_tracks_add, imgenv_scenarios_add and the features' enables
// allocate through, each committing to h->allocs once everything is there
struct HipApi {
    static const char* text(hipError_t e) { return e == hipSuccess ? nullptr : ((void)hipGetLastError(), hipGetErrorString(e)); }
    static const char* malloc(void** p, size_t bytes) { return text(hipMalloc(p, bytes)); }
    static const char* free(void* p) { return text(hipFree(p)); }
    static const char* memset(void* p, int byte, size_t bytes) { return text(hipMemset(p, byte, bytes)); }
    static const char* memcpy(void* dst, const void* src, size_t bytes, bool from_device) {
        return text(hipMemcpy(dst, src, bytes, from_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    }
};
// (the "after the first reset" refusals of imgenv_maps_add, imgenv_tracks_add and imgenv_stack_enable)
static bool any_world_reset(const imgenv* h) {
    bool any = h->has_reset;
    for (char r : h->world_ready) any = any || r;
    return any;
}
// (an error inside a create phase or a reset is handed up: imgenv_create destroys the half-built handle, a reset leaves it alive)
#define RTRY(expr)                   \
    do {                             \
        if (int rc_ = (expr)) return rc_; \
    } while (0)

extern "C" void imgenv_destroy(imgenv_t* h) {
    if (!h) return;
    for (void* p : h->allocs) (void)hipFree(p);
    if (h->comm && rccl_api()) (void)rccl_api()->destroy(h->comm);
    for (hipEvent_t e : h->t_ev) (void)hipEventDestroy(e);
    if (h->side) {
        (void)hipStreamSynchronize(h->side);
        (void)hipStreamDestroy(h->side);
    }
    if (h->side2) {
        (void)hipStreamSynchronize(h->side2);
        (void)hipStreamDestroy(h->side2);
    }
    if (h->err_host) (void)hipHostFree((void*)h->err_host);
    if (h->finished_host) (void)hipHostFree((void*)h->finished_host);
    for (int g = 0; g < imgenv::STAGE_GENS; g++) {
        for (auto& c : h->rs.chunks[g]) (void)hipHostFree(c.p);
        if (h->rs.ev_gen[g]) (void)hipEventDestroy(h->rs.ev_gen[g]);
    }
    if (h->dev.side3) {
        (void)hipStreamSynchronize(h->dev.side3);
        (void)hipStreamDestroy(h->dev.side3);
    }
    if (h->crowd.stream) {
        (void)hipStreamSynchronize(h->crowd.stream);
        (void)hipStreamDestroy(h->crowd.stream);
    }
    if (h->crowd.ev) (void)hipEventDestroy(h->crowd.ev);
    for (hipEvent_t e : h->crowd.ev_in)
        if (e) (void)hipEventDestroy(e);
    if (h->dev.ev_fill) (void)hipEventDestroy(h->dev.ev_fill);
    if (h->dev.ev_consumed) (void)hipEventDestroy(h->dev.ev_consumed);
    if (h->ev_fork2) (void)hipEventDestroy(h->ev_fork2);
    if (h->ev_join2) (void)hipEventDestroy(h->ev_join2);
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    if (h->ev_join) (void)hipEventDestroy(h->ev_join);
    if (h->own_arena && h->arena) (void)hipFree(h->arena);
    if (h->own_pub && h->pub_arena) (void)hipFree(h->pub_arena);
    delete h;
}

// ---------------------------------------------------------------------------------------- launch plans and kernel variants
// The kernel families that have template variants.  Each function names its family's instantiations ONCE (launch_plan.h: pick)
// and returns the chosen one: the launches go through here and so do imgenv_create's LDS attributes (lds_attributes), so a
// variant that can be launched has been given its LDS.
static auto k_raster_for(const PlanHandle& p, int nw) {
    decltype(&k_raster<true, 0, 1>) k = nullptr;
    pick([&](auto P2, auto LM, auto NW) { k = k_raster<P2(), LM(), NW()>; }, p.pow2, OneOf<0, 1, 2>{p.layer}, OneOf<1, 4>{nw});
    return k;
}
static auto k_move_raster_for(const PlanHandle& p, int nw) {
    decltype(&k_move_raster<true, 0, 1>) k = nullptr;
    pick([&](auto P2, auto LM, auto NW) { k = k_move_raster<P2(), LM(), NW()>; }, p.pow2, OneOf<0, 1, 2>{p.layer}, OneOf<1, 4>{nw});
    return k;
}
static auto k_raster_pack_for(const PlanHandle& p, int rpw) {
    decltype(&k_raster_pack<true, 2>) k = nullptr;
    pick([&](auto P2, auto RPW) { k = k_raster_pack<P2(), RPW()>; }, p.pow2, OneOf<2, 4>{rpw});
    return k;
}
static auto k_remote_for(const PlanHandle& p) { return p.pow2 ? k_remote<true> : k_remote<false>; }
static auto k_view_for(const PlanHandle& p, int nw) {
    decltype(&k_view<true, true, true, 1>) k = nullptr;
    pick([&](auto P2, auto A4, auto ST, auto NW) { k = k_view<P2(), A4(), ST(), NW()>; }, p.pow2, p.view_a4, p.layer == LAYER_STAMP, OneOf<1, 2, 4, 8>{nw});
    return k;
}
static auto k_crop_big_for(int sel) {  // (ViewPlan::crop_sel: <STAMP, TILED>, never tiled without the stamps)
    return sel == 2 ? k_crop_big<true, true> : sel == 1 ? k_crop_big<true, false> : k_crop_big<false, false>;
}
static auto k_beams_big_for(const PlanHandle& p) {
    decltype(&k_beams_big<true, true, true>) k = nullptr;
    pick([&](auto P2, auto ST, auto LB) { k = k_beams_big<P2(), ST(), LB()>; }, p.pow2, p.layer == LAYER_STAMP, p.big_bits_in_lds);
    return k;
}
static auto k_obs_for(const PlanHandle& p) {
    decltype(&k_obs<0>) k = nullptr;
    pick([&](auto E) { k = k_obs<E()>; }, OneOf<1, 2, 4, 8, 16, 0>{p.obs_E});
    return k;
}

// what the launch rules read of the handle, once imgenv_create has decided it
static void plan_facts(imgenv* h) {
    const DevWorld& d = h->d;
    PlanHandle& p = h->plan;
    p.R = h->R; p.RL = h->RL; p.P = h->P; p.W = h->W; p.Rw = h->Rw; p.Pw = h->Pw; p.NA = h->NA;
    p.sharded = d.sharded != 0; p.sum_shard = d.sum_shard != 0; p.pow2 = h->pow2;
    p.layer = h->stamp ? LAYER_STAMP : h->sum ? LAYER_SUM : LAYER_COMPOSED;
    p.serial = h->serial; p.big_view = h->big_view; p.view_a4 = h->geom.Wv % 4 == 0;
    p.B = d.B; p.lds_view = h->lds_view; p.lds_obs = h->lds_obs; p.lds_view_big = h->lds_view_big;
    p.obs_E = h->obs_E; p.n_sub = h->n_sub; p.relation = d.relation; p.scene = h->cfg.ped_scene_type;
    p.early = h->early; p.gates_work = h->gates_work;
    p.Gs = h->Gs; p.box_cells = d.box_cells;
    p.robot_classes = (int)h->rcls.size(); p.pack_rows = true; p.pack_bitmap_cells = 0; p.pack_force = h->raster_pack;
    p.obs_room_force = h->obs_room;
    for (const RobotClassHost& k : h->rcls) {  // (plan_raster_pack)
        const int side = 2 * k.box_rad + 1, bside = side - 4;
        p.pack_rows = p.pack_rows && !k.fp_rows.empty() && side * side <= d.box_cells;
        p.pack_bitmap_cells = std::max(p.pack_bitmap_cells, bside * bside);
    }
    p.big_max_crop = h->big_max_crop; p.big_full_chunks = h->big_full_chunks; p.big_tap_chunks_dyn = h->big_tap_chunks_dyn;
    p.big_bits_in_lds = h->big_bits_in_lds; p.crop_map = d.crop_map != nullptr;
    p.img_w = d.img_w; p.img_h = d.img_h; p.resize = d.resize != 0; p.keep_view_maps = d.keep_view_maps != 0;
}
// ... and of the chain of launches in hand (set_active has said what it covers)
static PlanChain chain_facts(const imgenv* h, int is_reset, bool moved = false, bool local_only = false) {
    static const bool early_off = getenv("IMGENV_EARLY_OBS") && atoi(getenv("IMGENV_EARLY_OBS")) == 0;  // (measurement switch)
    const DevWorld& d = h->d;
    PlanChain c;
    c.act_ng = d.act_ng; c.act_np = d.act_np; c.act_nl = d.act_nl; c.act_nw = d.act_nw; c.act_cells = d.act_cells;
    c.listed = d.act_list != nullptr; c.n_dev = d.act_n_dev != nullptr; c.act_hint = h->dev.act_hint;
    c.is_reset = is_reset != 0; c.moved = moved; c.local_only = local_only;
    c.stamp_seq = h->stamp_seq;
    c.orca_cap = std::max(h->cap_obst, d.n_obst);
    c.chain_open = h->step.chain_open; c.orca_ran = h->step.orca_seq > 0; c.view_ran = h->step.view_seq > 0; c.in_step = h->step.in_step;
    c.comm = h->comm != nullptr; c.crowd_ahead = h->crowd.can; c.early_off = early_off;
    return c;
}
// every variant of this handle that wants more than the default 64 KiB of LDS is allowed it
static int lds_attributes(imgenv* h) {
    const PlanHandle& p = h->plan;
    auto allow = [](const void* k, size_t bytes) -> int {
        if (bytes > LDS_DEFAULT_MAX) HIPCHK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        return 0;
    };
    if (p.big_view) {
        if (int rc = allow((const void*)k_taps_big, taps_lds_bytes(p.B))) return rc;
        if (int rc = allow((const void*)k_beams_big_for(p), p.lds_view_big)) return rc;
    }
    for (int nw : {1, 2, 4, 8})
        if (int rc = allow((const void*)k_view_for(p, nw), p.lds_view)) return rc;
    for (int rpw : {2, 4})
        if (int rc = allow((const void*)k_raster_pack_for(p, rpw), plan_raster_pack_lds(p, rpw))) return rc;
    // (k_obs beside packed rasters asks for more than it uses, plan_obs_lds: the size of a whole-handle early step)
    PlanChain whole;
    whole.act_ng = p.R; whole.act_np = p.P; whole.act_nl = p.RL;
    return allow((const void*)k_obs_for(p), std::max(p.lds_obs, plan_obs(p, whole, true).lds));
}

// view_big.h's one-byte-per-cell summary of a static map (world.h: crop_map), in 8 x 8 tiles
static void tile_crop(const uint8_t* map, int Hg, int Wg, uint32_t wt, size_t crop_ws, std::vector<uint8_t>& tiled) {
    tiled.assign(crop_ws, 0);
    for (int m = 0; m < Hg; m++)
        for (int n = 0; n < Wg; n++)
            tiled[(((size_t)(m >> 3) * wt + (n >> 3)) << 6) | ((m & 7) << 3) | (n & 7)] = map[(size_t)m * Wg + n] >= 250 ? 128 : 0;
}

// ---------------------------------------------------------------------------------------- create
// imgenv_create checks its arguments and plans (create_plan.h, out_fields.h: nothing of the device), then runs the phases below in
// order on the new handle.  A phase that fails returns its code; imgenv_create alone destroys the half-built handle, and
// imgenv_destroy copes with whatever the phases got to.  No allocation may change size, fill value or place in the order: the
// order decides the addresses.

// n zeroed ints of page-locked host memory that the device writes through (no copy, no sync to read them), and the device's pointer
static int mapped_ints(size_t n, volatile int** host, int** dev) {
    HIPCHK(hipHostMalloc((void**)host, n * sizeof(int), hipHostMallocMapped));
    memset((void*)*host, 0, n * sizeof(int));
    HIPCHK(hipHostGetDevicePointer((void**)dev, (void*)*host, 0));
    return 0;
}
static int chain_event(hipEvent_t* e) {
    HIPCHK(hipEventCreateWithFlags(e, hipEventDisableTiming | hipEventDisableSystemFence));
    return 0;
}
// world 0's copy of a layer to the other worlds: log2(W) device copies instead of W uploads
static int copy_to_worlds(uint8_t* layer, size_t stride, int W) {
    for (size_t filled = 1; filled < (size_t)W; filled *= 2)
        HIPCHK(hipMemcpy(layer + filled * stride, layer, std::min(filled, (size_t)W - filled) * stride, hipMemcpyDeviceToDevice));
    return 0;
}

// the robots' and pedestrians' classes (shape, size, sensor) and their host tables
static int create_classes(imgenv* h, const imgenv_cfg& c, const CreateArgs& a) {
    CreateMsg msg;
    if (int rc = create_check_shapes(c, msg)) FAIL(rc, "%s", msg);
    const int R = c.n_robots, P = c.n_peds;
    h->cfg = c;
    h->geom = a.g;
    h->robot_cls.resize(R);
    h->rsl.resize(R);
    for (int i = 0; i < R; i++) {
        const int shape = c.robot_shape[i];
        int found = -1;
        for (size_t q = 0; q < h->rcls.size(); q++)
            if (h->rcls[q].shape == shape && !memcmp(h->rcls[q].size, c.robot_size + 4 * i, 16) &&
                !memcmp(h->rcls[q].sensor, c.robot_sensor_cfg + 2 * i, 8))
                found = (int)q;
        if (found < 0) {
            RobotClassHost k;
            k.shape = shape;
            memcpy(k.size, c.robot_size + 4 * i, 16);
            memcpy(k.sensor, c.robot_sensor_cfg + 2 * i, 8);
            // tiled kernels (view_big.h): where k_view cannot run (its packing -- decided in build_robot_class -- or a shrunk
            // sensor_map) and on request.  (Measured on BASELINE cfg-5's 96 x 96 views, 8192 robots beside k_obs<16>: k_view
            // 471 us per step, the tiled kernels 531 -- the same instruction count in three launches; k_view stays the default
            // wherever it can run.)
            const bool tiled = a.view_resize || ((c.flags & IMGENV_FLAG_VIEW_TILED) && !(c.flags & IMGENV_FLAG_VIEW_WAVE));
            build_robot_class(k, a.g, tiled, (c.flags & IMGENV_FLAG_AGENT_STATE_EXTRAS) != 0);
            h->rcls.push_back(std::move(k));
            found = (int)h->rcls.size() - 1;
        }
        h->robot_cls[i] = found;
        h->rsl[i] = c.robot_size_last ? c.robot_size_last[i] : 0.0;
    }
    h->ped_cls.resize(P);
    h->pmax.resize(P);
    for (int j = 0; j < P; j++) {
        int found = -1;
        for (size_t q = 0; q < h->pcls.size(); q++)
            if (h->pcls[q].shape == c.ped_shape[j] && !memcmp(h->pcls[q].size, c.ped_size + 6 * j, 24)) found = (int)q;
        if (found < 0) {
            PedClassHost k;
            k.shape = c.ped_shape[j];
            memcpy(k.size, c.ped_size + 6 * j, 24);
            build_ped_class(k, a.g.res);
            h->pcls.push_back(std::move(k));
            found = (int)h->pcls.size() - 1;
        }
        h->ped_cls[j] = found;
        h->pmax[j] = c.ped_max_speed[j];
    }
    h->cfg.robot_shape = nullptr; h->cfg.robot_size = nullptr; h->cfg.robot_sensor_cfg = nullptr;
    h->cfg.ped_shape = nullptr; h->cfg.ped_size = nullptr; h->cfg.ped_max_speed = nullptr;
    h->cfg.robot_size_last = nullptr;
    return 0;
}

// what the plan says, into the handle and the kernels' DevWorld (no device call)
static void create_facts(imgenv* h, const CreatePlan& p, const uint8_t* static_map, int Hg_in, int Wg_in) {
    const imgenv_cfg& c = h->cfg;
    const ViewGeom& g = h->geom;
    const int W = p.W;
    h->serial = p.serial;  // (profiling aid: no side streams, clean per-kernel timings)
    if (const char* e = getenv("IMGENV_RASTER_PACK")) {  // (measurement switch, per handle: 0 never, 2 / 4 that many robots per wavefront)
        const int v = atoi(e);
        h->raster_pack = v == 2 || v == 4 ? v : 0;
    }
    if (const char* e = getenv("IMGENV_OBS_ROOM"))  // (measurement switch, per handle: 0 off, else the workgroups per compute unit k_obs leaves the packed rasters)
        h->obs_room = std::max(atoi(e), 0);
    h->R = p.R; h->P = p.P; h->r0 = p.r0; h->r1 = p.r1; h->RL = p.RL; h->NA = p.NA;
    h->Hg = p.Hg; h->Wg = p.Wg; h->Hg_in = Hg_in; h->Wg_in = Wg_in;
    h->map_stride = align16(p.G);
    h->W = W; h->Rw = p.Rw; h->Pw = p.Pw; h->Gs = p.Gs;
    h->world_epoch.assign(W, 0);
    h->world_ready.assign(W, 0);
    h->rvos.resize(W);
    h->wobst.assign((size_t)4 * W, 0);
    h->static_map.assign(static_map, static_map + p.G);
    h->pow2 = p.pow2; h->n_sub = p.n_sub;
    h->stamp = p.layer.stamp; h->sum = p.layer.sum;
    h->big_view = p.big_view; h->big_full_chunks = p.big_full_chunks; h->big_bits_in_lds = p.big_bits_in_lds;
    h->PP = p.PP; h->obs_E = p.obs_E;
    h->lds_view = p.lds_view; h->lds_obs = p.lds_obs; h->lds_view_big = p.lds_view_big;
    static_assert(PM_CAP * 2 <= WAVE * 7 * 4, "the touched-cell list reuses the staging buffer");
    h->crowd.can = p.sfm_ahead; h->early = p.early;
    h->arena_bytes = p.arena.total;

    DevWorld& d = h->d;
    memset(&d, 0, sizeof(d));
    d.R = p.R; d.RL = p.RL; d.r0 = p.r0; d.P = p.P; d.NA = p.NA;
    d.W = W; d.Rw = p.Rw; d.Pw = p.Pw; d.Gs = (uint32_t)p.Gs;
    d.act_list = nullptr; d.act_nw = W; d.act_nl = p.RL; d.act_ng = p.R; d.act_np = p.P;
    d.act_cells = W > 1 ? p.Gs * W : p.Gs;
    d.Hg = p.Hg; d.Wg = p.Wg; d.Hv = g.Hv; d.Wv = g.Wv; d.B = g.B;
    d.Hp = c.ped_image_size[0]; d.Wp = c.ped_image_size[1];
    d.SD = c.state_dim; d.PV = 1 + c.ped_vec_dim * c.max_ped;
    d.scene = c.ped_scene_type; d.relation = c.relation_ped_robo; d.ktype = c.robot_ktype;
    d.use_laser = c.use_laser ? 1 : 0; d.laser_norm = c.laser_norm; d.time_max = c.time_max;
    d.res = g.res; d.inv_res = 1.0 / g.res;
    d.wv_magic = p.wv_magic;
    d.step_hz = (double)c.step_hz; d.laser_max = c.laser_max;
    d.laser_out_nohit = c.laser_norm ? (double)6.0f / (double)c.laser_max : (double)6.0f;
    d.ped_safety_space = c.ped_safety_space; d.ped_image_r = c.ped_image_r;
    d.ped_image_r2 = pow(c.ped_image_r, 2.0);        // self.ped_image_r ** 2 (yaml_env.py:425)
    d.ped_res = p.ped_res; d.ped_inv_res = p.ped_inv_res;
    d.view_base = g.view_base; d.base_view = g.base_view;
    {   // SpeedLimiter(msg) (speed_limit.cpp:56-65): max_jerk <- msg.min_jerk, min_jerk uninitialised (0 here)
        const imgenv_limiter& v = c.limiter_v; const imgenv_limiter& ww = c.limiter_w;
        d.lv_has_v = v.has_velocity_limits; d.lv_has_a = v.has_acceleration_limits; d.lv_has_j = v.has_jerk_limits;
        d.lv_min_v = v.min_velocity; d.lv_max_v = v.max_velocity; d.lv_min_a = v.min_acceleration;
        d.lv_max_a = v.max_acceleration; d.lv_min_j = 0.0; d.lv_max_j = v.min_jerk;
        d.lw_has_v = ww.has_velocity_limits; d.lw_has_a = ww.has_acceleration_limits; d.lw_has_j = ww.has_jerk_limits;
        d.lw_min_v = ww.min_velocity; d.lw_max_v = ww.max_velocity; d.lw_min_a = ww.min_acceleration;
        d.lw_max_a = ww.max_acceleration; d.lw_min_j = 0.0; d.lw_max_j = ww.min_jerk;
    }
    const LayerPlan& l = p.layer;
    d.layer_sum = l.sum ? 1 : 0; d.sum_shard = l.sum_shard ? 1 : 0;
    d.sum_pc_mask = l.sum_pc_mask; d.sum_rc_shift = l.sum_rc_shift; d.sum_id_shift = l.sum_id_shift; d.sum_wg_magic = l.sum_wg_magic;
    d.rm_rad = l.rm_rad;
    d.stamp_tag = 1;
    d.resize = p.view_resize ? 1 : 0;
    d.img_w = c.image_size[0];
    d.img_h = c.image_size[1];
    d.keep_view_maps = (c.flags & IMGENV_FLAG_NO_VIEW_MAPS) ? 0 : 1;
    d.big_words = p.big_words; d.big_hit_stride = p.big_hit_stride;
    d.big_bits_in_lds = p.big_view && p.big_bits_in_lds ? 1 : 0;
    d.pd_cap = p.pd_cap; d.ped_box_cells = p.pd_cap;
    d.box_cells = p.box_cells; d.fp_cap = p.fp_cap;
    d.sharded = p.RL != p.R;
    d.region_margin = p.region_margin;
    d.beep_on = p.beep_on ? 1 : 0;
    d.beep_r = c.beep_r;
    d.ped_ca_p = (double)c.ped_ca_p;
    d.state_in_integrate = p.P == 0 ? 1 : 0;
    d.view_max_dist32 = c.view_max_dist;
    d.obs_passes = p.obs_passes;
    d.hit_stride = p.hit_stride;
}

// grids (one copy per world) and the class layer in the plan's mode
static int create_grid_layers(imgenv* h, const CreatePlan& p) {
    DevWorld& d = h->d;
    const int W = p.W;
    RTRY(dev_alloc(h, &h->d_obs_map, p.Gp));
    HIPCHK(hipMemcpy(h->d_obs_map, h->static_map.data(), p.G, hipMemcpyHostToDevice));
    RTRY(copy_to_worlds(h->d_obs_map, h->Gs, W));
    RTRY(dev_alloc(h, &h->d_static_map, align16(p.G)));
    HIPCHK(hipMemcpy(h->d_static_map, h->static_map.data(), p.G, hipMemcpyHostToDevice));
    RTRY(dev_alloc(h, &h->d_world_epoch, W));
    d.world_epoch = h->d_world_epoch;
    RTRY(dev_alloc(h, &h->d_wobst, (size_t)4 * W));
    d.obst_base = h->d_wobst; d.node_base = h->d_wobst + W; d.n_obst_w = h->d_wobst + 2 * W; d.oroot_w = h->d_wobst + 3 * W;
    d.obs_map = h->d_obs_map;
    if (d.sum_shard) {
        RTRY(dev_alloc(h, &d.rm_bits, (size_t)p.R));
        RTRY(dev_alloc(h, &d.rm_center, (size_t)p.R));
    }
    if (!h->stamp && !h->sum) {
        RTRY(dev_alloc(h, &d.ped_layer, p.Gp));
        RTRY(dev_alloc(h, &d.own_lo, p.Gp, 0xFF));
        RTRY(dev_alloc(h, &d.own_hi, p.Gp));
    }
    RTRY(dev_alloc(h, &d.cell, p.Gp));
    RTRY(dev_alloc(h, &d.seg_tag, p.Gp / 64 + 2));
    return 0;
}

// the classes' tables on the device, and what the kernels read per robot / pedestrian of its class
static int create_class_tables(imgenv* h, const CreatePlan& p) {
    DevWorld& d = h->d;
    const imgenv_cfg& c = h->cfg;
    std::vector<RobotClassDev> rc(h->rcls.size());
    for (size_t q = 0; q < h->rcls.size(); q++) {
        const RobotClassHost& k = h->rcls[q];
        RobotClassDev& o = rc[q];
        o.n_fp = k.fp.n();
        {
            std::vector<double2> fp(k.fp.n());
            for (int s = 0; s < k.fp.n(); s++) fp[s] = make_double2(k.fp.x[s], k.fp.y[s]);
            RTRY(dev_upload(h, &o.fp, fp));
        }
        RTRY(dev_upload(h, &o.fov_bits, k.fov_bits));
        RTRY(dev_upload(h, &o.stamp_bits, k.stamp_bits));
        o.ray_maxlen = k.ray_maxlen;
        o.ray_stride = k.ray_stride;
        o.ray_kpad = k.ray_kpad;
        RTRY(dev_upload(h, &o.ray_rows, k.ray_rows));
        RTRY(dev_upload(h, &o.ray_len, k.ray_len));
        RTRY(dev_upload(h, &o.ray_dist, k.ray_dist));
        if (!k.big) {  // what k_view needs of a beam's first hit, per (step, beam): the host's IEEE division = the device's
            std::vector<uint32_t> fin(4 * k.ray_dist.size());
            for (size_t s = 0; s < k.ray_dist.size(); s++) {
                const float hd = k.ray_dist[s];
                const double out = c.laser_norm ? (double)hd / (double)c.laser_max : (double)hd;
                fin[4 * s] = k.ray_run[s];
                memcpy(&fin[4 * s + 1], &hd, 4);
                memcpy(&fin[4 * s + 2], &out, 8);
            }
            const uint32_t* fin_dev = nullptr;
            RTRY(dev_upload(h, &fin_dev, fin));
            o.ray_fin = (const uint4*)fin_dev;
        }
        RTRY(dev_upload(h, &o.ray_run, k.ray_run));
        if (!k.ray_hx.empty()) {
            RTRY(dev_upload(h, &o.ray_hx, k.ray_hx));
            RTRY(dev_upload(h, &o.ray_hy, k.ray_hy));
            RTRY(dev_upload(h, &o.bin_start, k.bin_start));
        }
        RTRY(dev_upload(h, &o.inv_pack, k.inv_pack));
        RTRY(dev_upload(h, &o.inv_ent, k.inv_ent));
        RTRY(dev_upload(h, &o.top_ent, k.top_ent));
        RTRY(dev_upload(h, &o.dyn_groups, k.dyn_groups));
        o.n_dyn = (int)k.dyn_groups.size();
        RTRY(dev_upload(h, &o.all_groups, k.all_groups));
        {
            const uint32_t* cells2 = nullptr;
            RTRY(dev_upload(h, &cells2, k.inv_cell));
            o.inv_cell = (const uint2*)cells2;
        }
        o.big = k.big ? 1 : 0;
        o.box_rad = k.box_rad;
        o.n_rows = (int)k.fp_rows.size();
        o.rows = nullptr;
        o.fp_cy = k.fp_cy;
        if (o.n_rows) RTRY(dev_upload(h, &o.rows, k.fp_rows));
    }
    for (size_t q = 0; q < rc.size(); q++) d.rc[q] = rc[q];
    RTRY(dev_upload(h, &d.rc_mem, rc));
    std::vector<PedClassDev> pc(h->pcls.size());
    for (size_t q = 0; q < h->pcls.size(); q++) {
        const PedClassHost& k = h->pcls[q];
        PedClassDev& o = pc[q];
        memset(&o, 0, sizeof(o));
        o.shape = k.shape;
        o.n_bbox = k.bbox.n();
        o.n_left = k.left.n();
        o.n_right = k.right.n();
        RTRY(dev_upload(h, &o.bx, k.bbox.x));
        RTRY(dev_upload(h, &o.by, k.bbox.y));
        RTRY(dev_upload(h, &o.lx, k.left.x));
        RTRY(dev_upload(h, &o.ly, k.left.y));
        RTRY(dev_upload(h, &o.rx, k.right.x));
        RTRY(dev_upload(h, &o.ry, k.right.y));
        memcpy(o.sizes, k.sizes, sizeof(o.sizes));
        o.box_rad = k.box_rad;
        o.n_brows = (int)k.bbox_rows.size(); o.n_lrows = (int)k.left_rows.size(); o.n_rrows = (int)k.right_rows.size();
        o.bbox_cy = k.bbox_cy;
        if (o.n_brows) RTRY(dev_upload(h, &o.brows, k.bbox_rows));
        if (o.n_lrows) RTRY(dev_upload(h, &o.lrows, k.left_rows));
        if (o.n_rrows) RTRY(dev_upload(h, &o.rrows, k.right_rows));
    }
    for (size_t q = 0; q < pc.size(); q++) d.pc[q] = pc[q];
    if (pc.empty()) pc.resize(1);
    RTRY(dev_upload(h, &d.pc_mem, pc));
    RTRY(dev_upload(h, &d.robot_cls, h->robot_cls));
    RTRY(dev_upload(h, &d.ped_cls, h->ped_cls));
    RTRY(dev_upload(h, &d.robot_size_last, h->rsl));
    std::vector<double> pr_round(p.P);
    std::vector<float> pr32(p.P);
    for (int j = 0; j < p.P; j++) {
        pr32[j] = (float)h->pcls[h->ped_cls[j]].sizes[2];
        pr_round[j] = py_round2((double)pr32[j]);
    }
    RTRY(dev_upload(h, &d.ped_r_round, pr_round));
    RTRY(dev_upload(h, &d.ped_r32, pr32));
    std::vector<uint16_t> lut(256);
    for (int v = 0; v < 256; v++) lut[v] = f32_to_f16((float)v / 255.0f);  // numpy: f16(f32(v)/255)
    RTRY(dev_upload(h, &d.f16_lut, lut));
    return 0;
}

// the shrunk sensor_map's axis tables, and what the tiled kernels of view_big.h need
static int create_view_tables(imgenv* h, const CreatePlan& p) {
    DevWorld& d = h->d;
    const ViewGeom& g = h->geom;
    const int W = p.W, Hg = p.Hg, Wg = p.Wg, RL = p.RL;
    CvAxis ax, ay;
    if (p.view_resize) {  // axis tables of the bicubic shrink (csrc/cv_resize.h)
        ax = cv_axis(g.Wv, d.img_w, true, true);
        ay = cv_axis(g.Hv, d.img_h, true, false);
        RTRY(dev_upload(h, &d.rs_xofs, ax.ofs));
        RTRY(dev_upload(h, &d.rs_alpha, ax.coef));
        RTRY(dev_upload(h, &d.rs_yofs, ay.ofs));
        RTRY(dev_upload(h, &d.rs_beta, ay.coef));
    }
    if (!h->big_view) return 0;
    // view_big.h: tiled crop bitmap + hit words per local robot, static tables per class
    if (h->stamp && p.G < ((size_t)1 << 24)) {  // view_big.h: the map as k_crop_big wants it (world.h)
        const uint32_t wt = (uint32_t)(Wg + 7) / 8, ht = (uint32_t)(Hg + 7) / 8;
        d.crop_wt = wt;
        d.crop_ws = wt * ht * 64;
        d.crop_magic = (((unsigned long long)1 << 40) + (unsigned long long)Wg - 1) / (unsigned long long)Wg;
        for (int m = 0; m < Hg; m++)  // (the multiply-shift division is exact on this map: row starts and row ends)
            for (int e = 0; e < 2; e++) {
                const unsigned long long cl = (unsigned long long)m * Wg + (e ? Wg - 1 : 0);
                if ((int)((cl * d.crop_magic) >> 40) != m) FAIL(IMGENV_EINVAL, "internal: row of cell %llu by multiply-shift", cl);
            }
        std::vector<uint8_t> tiled;
        tile_crop(h->static_map.data(), Hg, Wg, wt, (size_t)d.crop_ws, tiled);
        uint8_t* sc = nullptr;
        RTRY(dev_alloc(h, &sc, (size_t)d.crop_ws));
        HIPCHK(hipMemcpy(sc, tiled.data(), tiled.size(), hipMemcpyHostToDevice));
        d.static_crop = sc;
        RTRY(dev_alloc(h, &d.crop_map, (size_t)d.crop_ws * W));
        HIPCHK(hipMemcpy(d.crop_map, sc, (size_t)d.crop_ws, hipMemcpyDeviceToDevice));
        RTRY(copy_to_worlds(d.crop_map, d.crop_ws, W));
    }
    std::vector<BigClassDev> bc(h->rcls.size());
    int max_crop = 1;
    for (size_t q = 0; q < h->rcls.size(); q++) {
        RobotClassHost& k = h->rcls[q];
        BigClassDev& o = bc[q];
        memset(&o, 0, sizeof(o));
        o.ta = k.big_ta;
        o.tb = k.big_tb;
        o.n_crop = k.n_crop;
        max_crop = std::max(max_crop, o.n_crop);
        RTRY(dev_upload(h, &o.crop_tiles, k.crop_tiles));
        RTRY(dev_upload(h, &o.crop_masks, k.crop_masks));
        RTRY(dev_upload(h, &o.cells, k.big_cells));
        RTRY(dev_upload(h, &o.ray_end, k.ray_end));
        {
            const uint32_t* p2 = nullptr;
            RTRY(dev_upload(h, &p2, k.big_inv));
            o.inv = (const uint2*)p2;
        }
        if (p.view_resize) {
            build_big_taps(k, g, ax.ofs, ay.ofs);
            const uint32_t* p2i = nullptr;
            RTRY(dev_upload(h, &o.tap_top, k.tap_top));
            RTRY(dev_upload(h, &p2i, k.tap_inv));
            o.tap_inv = (const uint2*)p2i;
            RTRY(dev_upload(h, &o.tap_addr, k.tap_addr));
            RTRY(dev_upload(h, &o.tap_chunks, k.tap_chunks));
            o.n_tap_chunks = (int)k.tap_chunks.size();
            h->big_tap_chunks_dyn = std::max(h->big_tap_chunks_dyn, o.n_tap_chunks);
            std::vector<uint32_t>().swap(k.tap_top);
            std::vector<uint32_t>().swap(k.tap_inv);
            std::vector<uint32_t>().swap(k.tap_addr);
        }
    }
    for (size_t q = 0; q < bc.size(); q++) d.big[q] = bc[q];
    RTRY(dev_alloc(h, &d.big_bits, (size_t)RL * 2 * d.big_words));
    RTRY(dev_alloc(h, &d.big_hit, (size_t)RL * d.big_hit_stride));
    // cells no crop tile covers lie outside the field of view for good: "unknown" in plane 1 (read without the laser only)
    if (!h->cfg.use_laser)
        HIPCHK(hipMemset2D(d.big_bits + d.big_words, (size_t)8 * d.big_words, 0xFF, (size_t)4 * d.big_words, (size_t)RL));
    h->big_max_crop = max_crop;
    return 0;
}

// robot / pedestrian / RVO state, the beep lottery, the flags the device raises
static int create_agents(imgenv* h, const CreatePlan& p) {
    DevWorld& d = h->d;
    const int R = p.R, P = p.P, RL = p.RL, NA = p.NA, W = p.W;
    RTRY(dev_alloc(h, &d.gx, RL)); RTRY(dev_alloc(h, &d.gy, RL));
    RTRY(dev_alloc(h, &d.l0v, RL)); RTRY(dev_alloc(h, &d.l0w, RL)); RTRY(dev_alloc(h, &d.l1v, RL)); RTRY(dev_alloc(h, &d.l1w, RL));
    RTRY(dev_alloc(h, &d.world_target, RL));
    RTRY(dev_alloc(h, &d.is_coll, RL)); RTRY(dev_alloc(h, &d.is_arr, RL)); RTRY(dev_alloc(h, &d.py_done, RL));
    RTRY(dev_alloc(h, &d.clean_state, RL, 1));
    RTRY(dev_alloc(h, &d.tmp_dist, RL));
    RTRY(dev_alloc(h, &d.pm_cells, (size_t)RL * PM_CAP));
    RTRY(dev_alloc(h, &d.pm_n, RL));  // 0: the arena starts zeroed, nothing to clear
    if (h->sum) {  // every pedestrian keeps the list of the cells it counts itself on
        RTRY(dev_alloc(h, &d.pd_cells, (size_t)(P > 0 ? P : 1) * d.pd_cap));
        RTRY(dev_alloc(h, &d.pd_n, P > 0 ? P : 1));
    }
    RTRY(dev_alloc(h, &d.bbox, 4));
    RTRY(dev_alloc(h, &d.fp_cells, (size_t)RL * d.fp_cap));
    RTRY(dev_alloc(h, &d.fp_n, RL, 0xFF));  // -1 until the first raster
    RTRY(dev_alloc(h, &d.fp_pose, (size_t)RL * 3));
    RTRY(dev_alloc(h, &d.ppx, P)); RTRY(dev_alloc(h, &d.ppy, P)); RTRY(dev_alloc(h, &d.pyaw, P));
    RTRY(dev_alloc(h, &d.plx, P)); RTRY(dev_alloc(h, &d.ply, P)); RTRY(dev_alloc(h, &d.pvx, P)); RTRY(dev_alloc(h, &d.pvy, P));
    RTRY(dev_alloc(h, &d.prem, P)); RTRY(dev_alloc(h, &d.llx, P)); RTRY(dev_alloc(h, &d.lly, P));
    RTRY(dev_alloc(h, &d.rlx, P)); RTRY(dev_alloc(h, &d.rly, P));
    RTRY(dev_alloc(h, &d.pstate, P)); RTRY(dev_alloc(h, &d.ptraj_idx, P));
    RTRY(dev_alloc(h, &h->d_traj_len, P));
    d.ptraj_len = h->d_traj_len;
    RTRY(dev_alloc(h, &d.apx, NA)); RTRY(dev_alloc(h, &d.apy, NA)); RTRY(dev_alloc(h, &d.avx, NA)); RTRY(dev_alloc(h, &d.avy, NA));
    RTRY(dev_alloc(h, &d.anvx, NA)); RTRY(dev_alloc(h, &d.anvy, NA));
    RTRY(dev_alloc(h, &d.near_n, P)); RTRY(dev_alloc(h, &d.near_list, (size_t)(P > 0 ? P : 1) * ORCA_NEAR_CAP));
    {
        std::vector<float> ms(NA > 0 ? NA : 1, 0.6f);  // robots: maxSpeed 0.6 (rvoscene.h:63)
        for (int j = 0; j < P && j < NA; j++) ms[j] = (float)(double)h->pmax[j];
        RTRY(dev_upload(h, &d.amax_speed, ms));
    }
    if (p.beep_on) {  // one rand() stream per world = per node process of the reference, as a fresh process starts it
        uint32_t s0[31];
        beep_initial_state(s0);
        std::vector<uint32_t> st((size_t)31 * W);
        for (int k = 0; k < W; k++) memcpy(&st[(size_t)31 * k], s0, sizeof(s0));
        const uint32_t* up = nullptr;
        RTRY(dev_upload(h, &up, st));
        d.beep_state = const_cast<uint32_t*>(up);
        RTRY(dev_upload(h, &d.beep_coef, beep_coefficients(BEEP_T)));
        RTRY(dev_alloc(h, &d.beep_flag, R));
        RTRY(dev_alloc(h, &d.beep_xy, R));
    }
    // the finished-world list of imgenv_step_autoreset: written by k_finished straight into page-locked host memory
    RTRY(mapped_ints((size_t)(1 + W), &h->finished_host, &d.finished));
    // overflow flags live in page-locked host memory the device writes through: no copy, no sync to read them
    RTRY(mapped_ints(8, &h->err_host, &d.err));
    d.sfm.err = d.err + 4;
    return 0;
}

// the social-force crowd: PedScene(): Tscene(0,10,10,10), addPed, addRobot (pedscene.h:17-80)
static int create_crowd(imgenv* h, const CreatePlan& p) {
    const imgenv_cfg& c = h->cfg;
    if (c.ped_scene_type != IMGENV_SCENE_PEDSIM) return 0;
    // one crowd per world (the reference: one node process = one PedScene per env), every array W slices back to back;
    // every world starts as a fresh process does: the same default-seeded draws
    SfmDev& f = h->d.sfm;
    const int Pw = p.Pw, Rw = p.Rw, W = p.W;
    const int n = Pw + (c.relation_ped_robo == 1 ? Rw : 0), n1 = n ? n : 1;
    f.n = n; f.n_peds = Pw; f.n_obs = 0; f.W = W;
    f.cap_nodes = W > 1 ? 2048 : 16384;  // (libpedsim's tree only ever grows: a crowd that outgrows its pool raises the overflow flag)
    f.cap_obs = 0;
    PedsimRng rng;
    std::vector<double> p0((size_t)n1 * 3, 0.0), vmax(n1, 0.0);
    std::vector<SfmNode> nodes(f.cap_nodes);
    std::vector<int> treehash(n1, 0);
    int n_nodes = 0, err = 0;
    sfm_q_new(nodes.data(), &n_nodes, f.cap_nodes, 0, 10, 10, 10);
    // every Tagent() draws its vmax (peds then robots, also robots that stay outside the scene)
    for (int a = 0; a < n; a++) {
        vmax[a] = rng.normal_fresh(1.2, 0.2);
        if (a < Pw) {
            p0[3 * a] = rng.glibc_rand() / 2147483647.0 * 10.0;
            p0[3 * a + 1] = rng.glibc_rand() / 2147483647.0 * 10.0;
            vmax[a] = (double)h->pmax[a];
        }
        sfm_add_agent(nodes.data(), &n_nodes, f.cap_nodes, treehash.data(), p0.data(), a, &err);
    }
    if (err) FAIL(IMGENV_EINVAL, "pedscene quadtree construction overflowed (%d)", err);
    const size_t Wn = (size_t)W * n1;
    RTRY(dev_alloc(h, &f.p, Wn * 3));
    RTRY(dev_alloc(h, &f.v, Wn * 3));
    RTRY(dev_alloc(h, &f.vmax, Wn)); RTRY(dev_alloc(h, &f.wpx, Wn * SFM_MAX_WP));
    RTRY(dev_alloc(h, &f.wpy, Wn * SFM_MAX_WP)); RTRY(dev_alloc(h, &f.wpr, Wn * SFM_MAX_WP));
    RTRY(dev_alloc(h, &f.dq, Wn * SFM_MAX_WP)); RTRY(dev_alloc(h, &f.dq_n, Wn));
    RTRY(dev_alloc(h, &f.dest, Wn, 0xFF)); RTRY(dev_alloc(h, &f.last, Wn, 0xFF));  // -1
    RTRY(dev_alloc(h, &f.nodes, (size_t)W * f.cap_nodes)); RTRY(dev_alloc(h, &f.n_nodes, W)); RTRY(dev_alloc(h, &f.treehash, Wn));
    RTRY(dev_alloc(h, &f.pair_f, (size_t)W * n1 * n1 * 3)); RTRY(dev_alloc(h, &f.pair_code, (size_t)W * n1 * n1));
    RTRY(dev_alloc(h, &f.g_nb, (size_t)W * SFM_MAX_AGENTS * (SFM_MAX_AGENTS / 32))); RTRY(dev_alloc(h, &f.g_sh, (size_t)W * 4 * SFM_MAX_AGENTS));
    if (W > 1) {  // room for every world's obstacle segments up front (a slice cannot grow without moving the others)
        f.cap_obs = 64;
        int* nobs = nullptr;
        RTRY(dev_alloc(h, &f.obs, (size_t)W * f.cap_obs * 4));
        RTRY(dev_alloc(h, &nobs, W));
        f.n_obs_w = nobs;
        h->sfm_cap_obs = f.cap_obs;
        h->sfm_nobs_w.assign(W, 0);
    }
    f.p_out = f.p; f.v_out = f.v; f.dq_out = f.dq; f.dest_out = f.dest; f.last_out = f.last;  // (a step in place)
    f.nodes_out = f.nodes; f.n_nodes_out = f.n_nodes; f.treehash_out = f.treehash;
    if (h->crowd.can) {
        SfmDev& o = h->crowd.other;
        o = f;
        RTRY(dev_alloc(h, &o.p, Wn * 3)); RTRY(dev_alloc(h, &o.v, Wn * 3));
        RTRY(dev_alloc(h, &o.dq, Wn * SFM_MAX_WP)); RTRY(dev_alloc(h, &o.dest, Wn, 0xFF)); RTRY(dev_alloc(h, &o.last, Wn, 0xFF));
        RTRY(dev_alloc(h, &o.nodes, (size_t)W * f.cap_nodes)); RTRY(dev_alloc(h, &o.n_nodes, W)); RTRY(dev_alloc(h, &o.treehash, Wn));
        HIPCHK(hipStreamCreateWithFlags(&h->crowd.stream, hipStreamNonBlocking));
        RTRY(chain_event(&h->crowd.ev));
        RTRY(chain_event(&h->crowd.ev_in[0]));
        RTRY(chain_event(&h->crowd.ev_in[1]));
    }
    for (int k = 0; k < W; k++) {
        HIPCHK(hipMemcpy(f.p + (size_t)k * n1 * 3, p0.data(), sizeof(double) * 3 * n1, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(f.vmax + (size_t)k * n1, vmax.data(), sizeof(double) * n1, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(f.nodes + (size_t)k * f.cap_nodes, nodes.data(), sizeof(SfmNode) * n_nodes, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(f.n_nodes + k, &n_nodes, sizeof(int), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(f.treehash + (size_t)k * n1, treehash.data(), sizeof(int) * n1, hipMemcpyHostToDevice));
    }
    return 0;
}

// the chain's scratch, the output arena (out_fields.h has its arrays) and the guards over it
static int create_outputs(imgenv* h, const CreatePlan& p) {
    DevWorld& d = h->d;
    const imgenv_cfg& c = h->cfg;
    const ViewGeom& g = h->geom;
    const ArenaLayout& lay = p.arena;
    const int RL = p.RL;
    RTRY(dev_alloc(h, &d.prof, 16 + 12 * (size_t)RL));
    RTRY(dev_alloc(h, &d.tail_sig, RL));
    RTRY(dev_alloc(h, &d.tail_cnt, (size_t)(RL + WAVE - 1) / WAVE * TAIL_CNT_STRIDE));
    RTRY(dev_alloc(h, &d.dbg, 32));  // phase sums | per-wave (start, end, hw id, -) of k_view and k_obs

    if (p.full_rewrite) {  // the caller's arena (or a second allocation) only ever receives copies; the kernels work on a private one
        if (c.out_arena) {
            h->pub_arena = (unsigned char*)c.out_arena;
        } else {
            void* pub = nullptr;
            if (hipMalloc(&pub, lay.total) != hipSuccess) FAIL(IMGENV_ENOMEM, "hipMalloc(%zu) for the public output arena failed", lay.total);
            h->pub_arena = (unsigned char*)pub;
            h->own_pub = true;
        }
        HIPCHK(hipMemset(h->pub_arena, 0, lay.total));
    }
    if (c.out_arena && !p.full_rewrite) {
        h->arena = (unsigned char*)c.out_arena;
    } else {
        void* own = nullptr;
        hipError_t e = hipMalloc(&own, lay.total);
        if (e != hipSuccess) FAIL(IMGENV_ENOMEM, "hipMalloc(%zu) for the output arena failed: %s", lay.total, hipGetErrorString(e));
        h->arena = (unsigned char*)own;
        h->own_arena = true;
    }
    HIPCHK(hipMemset(h->arena, 0, lay.total));
    unsigned char* A = h->arena;
    imgenv_out& o = h->out;
    o.struct_size = (int32_t)sizeof(imgenv_out);
    o.n_local = RL; o.view_h = g.Hv; o.view_w = g.Wv; o.n_beams = g.B; o.state_dim = c.state_dim; o.ped_vec_len = d.PV;
    o.image_h = d.img_h; o.image_w = d.img_w; o.grid_h = p.Hg; o.grid_w = p.Wg;
    // every array's pointer into imgenv_out and, under the same name, into DevWorld (the records: DevWorld alone)
    const bool extras = p.out.extras && p.out.has_beams;
#define OUT_PTR(name, bytes) d.name = o.name = (decltype(o.name))(A + lay.off[OUTF_##name]);
#define OUT_PTR_EXTRA(name, bytes) d.name = o.name = extras ? (decltype(o.name))(A + lay.off[OUTF_##name]) : nullptr;
#define OUT_PTR_HIDDEN(name, bytes) d.rec = (double*)(A + lay.off[OUTF_##name]);
    OUT_FIELDS(OUT_PTR, OUT_PTR_EXTRA, OUT_PTR_HIDDEN)
#undef OUT_PTR
#undef OUT_PTR_EXTRA
#undef OUT_PTR_HIDDEN
    {   // NearbyPed starts at +inf and is never re-initialised (reset_helper.py:85-99); is_clean starts True
        std::vector<double> inf(RL, INFINITY);
        HIPCHK(hipMemcpy(o.ped_min_dists, inf.data(), sizeof(double) * RL, hipMemcpyHostToDevice));
        HIPCHK(hipMemset(o.is_clean, 1, RL));
    }
    if (p.full_rewrite) {  // the same struct with every pointer moved into the public arena
        h->pub_out = o;
        const ptrdiff_t shift = h->pub_arena - h->arena;
#define OUT_SHIFT(name, bytes) \
    if (o.name) h->pub_out.name = (decltype(o.name))((unsigned char*)o.name + shift);
#define OUT_STAYS(name, bytes)
        OUT_FIELDS(OUT_SHIFT, OUT_SHIFT, OUT_STAYS)
#undef OUT_SHIFT
#undef OUT_STAYS
    }
    if (c.flags & (IMGENV_FLAG_CHECK_OUTPUTS | IMGENV_FLAG_CHECK_OUTPUTS_FIRST)) {  // every array of imgenv_out (not the records: the caller's exchange writes those)
        if (!(c.flags & IMGENV_FLAG_CHECK_OUTPUTS)) h->guard_left = IMGENV_CHECK_FIRST_CALLS;
        OutFieldRow rows[OUTF_COUNT];
        out_field_rows(p.out, rows);
        std::vector<OutSpan> spans;
        int blocks = 0;
        for (int q = 0; q < OUTF_COUNT; q++) {
            if (!rows[q].guarded || !out_field_exists(p.out, rows[q])) continue;
            OutSpan sp;
            sp.p = A + lay.off[q];
            sp.bytes = lay.slot(q);  // (the padding up to the next array is zero and stays zero)
            sp.first_block = blocks;
            blocks += (int)((sp.bytes + OUT_SUM_CHUNK - 1) / OUT_SUM_CHUNK);
            h->span_name[spans.size()] = rows[q].name;
            spans.push_back(sp);
        }
        h->n_spans = (int)spans.size();
        h->span_blocks = blocks;
        const OutSpan* up = nullptr;
        RTRY(dev_upload(h, &up, spans));
        h->d_spans = const_cast<OutSpan*>(up);
        RTRY(dev_alloc(h, &h->d_sums, 2 * (size_t)h->n_spans));
        h->guard_check = true;
    }
    return 0;
}

// what the observation kernel keeps between steps, and the snapshots of an early-observation step
static int create_obs_state(imgenv* h, const CreatePlan& p) {
    DevWorld& d = h->d;
    const int RL = p.RL, P = p.P;
    if (h->obs_E >= 2) {
        // last step's pedestrian order per robot (k_obs): any permutation of the slots will do to start from
        std::vector<uint16_t> ident((size_t)h->PP);
        for (int q = 0; q < h->PP; q++) ident[q] = q < h->Pw ? (uint16_t)q : (uint16_t)0xFFFF;
        RTRY(dev_alloc(h, &d.obs_ord, (size_t)RL * h->PP));
        std::vector<uint16_t> all((size_t)RL * h->PP);
        for (int r = 0; r < RL; r++) memcpy(&all[(size_t)r * h->PP], ident.data(), sizeof(uint16_t) * (size_t)h->PP);
        HIPCHK(hipMemcpy(d.obs_ord, all.data(), sizeof(uint16_t) * all.size(), hipMemcpyHostToDevice));
    }
    if (h->cfg.ped_scene_type == IMGENV_SCENE_PEDSIM)
        HIPCHK(hipFuncSetAttribute((const void*)k_sfm, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(SfmNode) * SFM_LDS_NODES)));
    // The early k_obs (where: plan_early_obs) always waits behind the GATE (world.h: sync): it reads the step's actions and REWRITES
    // output arrays, so it must run behind everything the caller queued on its stream in front of the step -- a policy that writes the actions, a
    // copy of the last observation into a replay buffer, FULL_REWRITE's own copy.  (Rounds 4-5 also had an ungated variant for
    // callers that promised complete actions, IMGENV_STEP_ACTIONS_READY; it only waited for the last chain's views, which does
    // not cover readers of the outputs -- and measured the same as the gate, 92.0 against 92.3 us per step.  Dropped in round 6.)
    if (h->early) {
        RTRY(dev_alloc(h, &d.sync, 8));
        RTRY(dev_alloc(h, &h->rec_snap[0], (size_t)RL * IMGENV_RECORD_DOUBLES));
        RTRY(dev_alloc(h, &h->rec_snap[1], (size_t)RL * IMGENV_RECORD_DOUBLES));
        RTRY(dev_alloc(h, &h->ped_snap[0], (size_t)(h->NA > 0 ? P : 1)));
        RTRY(dev_alloc(h, &h->ped_snap[1], (size_t)(h->NA > 0 ? P : 1)));
    }
    return 0;
}

// side streams, the gate probe, the chain's events, the launch rules' facts and the kernels' LDS
static int create_streams(imgenv* h, const CreatePlan& p) {
    DevWorld& d = h->d;
    HIPCHK(hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking));
    // (Round 6 tried the observation's stream on a subset of the compute units, hipExtStreamCreateWithCUMask, so that the move's
    // successors find free units at once: such a stream is a BLOCKING one -- it serialises against a caller on the null stream, 95 ->
    // 213 us per step whatever the mask -- and beside a caller on a stream of its own 24 / 28 / 16 of an XCD's 32 units cost 99.2 /
    // 99.5 / 108.3 us against 95.5: the step is bound by the instructions it issues, not by where they run.  docs/HISTORY.md)
    HIPCHK(hipStreamCreateWithFlags(&h->side2, hipStreamNonBlocking));
    if (h->early) {  // gates (world.h: sync) only where kernels of two streams really run side by side: k_gate_probe
        static int gates_work = -1;  // (per process)
        if (gates_work < 0) {
            k_gate_probe<<<dim3(1), dim3(WAVE), 0, h->side2>>>(d.sync + 2);
            k_gate_probe_set<<<dim3(1), dim3(1), 0, h->side>>>(d.sync + 2);
            HIPCHK(hipStreamSynchronize(h->side2));
            HIPCHK(hipStreamSynchronize(h->side));
            uint32_t verdict = 0;
            HIPCHK(hipMemcpy(&verdict, d.sync + 3, sizeof(verdict), hipMemcpyDeviceToHost));
            gates_work = verdict == 1u ? 1 : 0;
        }
        h->gates_work = gates_work == 1;
    }
    d.view_prio = (p.P == 0 || (h->early && h->gates_work && h->NA > 0 && h->obs_E >= 1 && h->obs_E <= 4)) ? 1 : 0;  // (world.h)
    RTRY(chain_event(&h->ev_fork2));
    RTRY(chain_event(&h->ev_join2));
    RTRY(chain_event(&h->ev_fork));
    RTRY(chain_event(&h->ev_join));
    plan_facts(h);
    RTRY(lds_attributes(h));
    HIPCHK(hipDeviceSynchronize());
    return 0;
}

extern "C" int imgenv_create(const imgenv_cfg* cfg, const uint8_t* static_map, int32_t Hg, int32_t Wg,
                             imgenv_t** out) {
    CreateMsg msg;
    CreateArgs a;
    if (int rc = create_check_args(cfg, static_map != nullptr, out != nullptr, Hg, Wg, a, msg)) FAIL(rc, "%s", msg);
    const int Hg_in = Hg, Wg_in = Wg;
    if (int rc = create_grid_size(*cfg, a.W, Hg, Wg, msg)) FAIL(rc, "%s", msg);
    std::vector<uint8_t> resized_map;
    if (cfg->global_resolution != cfg->view_resolution) {  // GridMap::read_image (grid_map.cpp:28-38)
        resized_map.resize((size_t)Hg * Wg);
        cv_resize_u8(false, static_map, Hg_in, Wg_in, resized_map.data(), Hg, Wg);
        static_map = resized_map.data();
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) FAIL(IMGENV_EDEVICE, "no HIP device available");
    if (cfg->device < 0 || cfg->device >= ndev) FAIL(IMGENV_EDEVICE, "device %d out of range (%d)", cfg->device, ndev);
    HIPCHK(hipSetDevice(cfg->device));
    const bool serial = getenv("IMGENV_SERIAL") && getenv("IMGENV_SERIAL")[0] == '1';

    imgenv* h = new imgenv();
    CreatePlan plan;
    int rc = create_classes(h, *cfg, a);
    if (!rc && (rc = plan_create(*cfg, a, Hg, Wg, serial, h->rcls, h->pcls, plan, msg))) snprintf(g_err, sizeof(g_err), "%s", msg);
    if (!rc) create_facts(h, plan, static_map, Hg_in, Wg_in);
    static int (*const phases[])(imgenv*, const CreatePlan&) = {create_grid_layers, create_class_tables, create_view_tables, create_agents,
                                                                create_crowd,       create_outputs,      create_obs_state,   create_streams};
    for (auto phase : phases)
        if (!rc) rc = phase(h, plan);
    if (rc) {  // the one owner of the half-built handle
        imgenv_destroy(h);
        return rc;
    }
    *out = h;
    return IMGENV_OK;
}

// ---------------------------------------------------------------------------------------- reset
// the t-th robot of a reset (list order): pose3 / rr hold the reset's robots in that order, in page-locked host memory
__device__ __forceinline__ void reset_robot(const DevWorld& w, const int* list, int t, const double* __restrict__ pose3,
                                            const ResetRobot* __restrict__ rr, int whole) {
    const int i = list ? list[t / w.Rw] * w.Rw + t % w.Rw : t;
    double* r = w.rec + (size_t)i * IMGENV_RECORD_DOUBLES;
    r[0] = pose3[5 * t];  // init_pose (agent.cpp:133-142); Agent::vx, vy persist across resets
    r[1] = pose3[5 * t + 1];
    r[2] = pose3[5 * t + 2];
    r[5] = pose3[5 * t + 3];  // sin / cos of yaw/2, evaluated on the host
    r[6] = pose3[5 * t + 4];
    const int l = i - w.r0;
    if (l >= 0 && l < w.RL) {
        const ResetRobot q = rr[w.W > 1 ? t : l];
        w.l0v[l] = 0;  // last0_vw_ = (0,0); last1_vw_ is not touched by init_pose
        w.l0w[l] = 0;
        w.gx[l] = q.gx;
        w.gy[l] = q.gy;
        w.world_target[l] = q.world_target;
        w.is_coll[l] = 0;
        w.is_arr[l] = 0;
    }
    if (t == 0 && whole) w.counters[2] = 0;  // frozen robot-steps since this reset (of every world)
}

// reset of a robot-sharded world: bounding box of the local robots' new positions (tail_group re-arms it every step)
__global__ void k_reset_bbox(DevWorld w, const double* __restrict__ pose3) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = l < w.RL;
    const double* p = pose3 + 5 * (size_t)(w.r0 + (valid ? l : 0));
    bbox_accumulate(w, valid, p[0], p[1]);
}

__device__ __forceinline__ void reset_ped(const DevWorld& w, const int* list, int t, const double* __restrict__ pose3) {
    const int j = list ? list[t / w.Pw] * w.Pw + t % w.Pw : t;
    const double x = pose3[3 * t], y = pose3[3 * t + 1];
    w.ppx[j] = x;
    w.ppy[j] = y;
    w.pyaw[j] = pose3[3 * t + 2];
    w.ptraj_idx[j] = 0;
    if (w.NA > 0) {  // setPedPos (rvoscene.h:32-34); the agent's velocity persists
        w.apx[j] = (float)x;
        w.apy[j] = (float)y;
    }
    if (w.scene == IMGENV_SCENE_PEDSIM) {  // setPosition(x, y, 0) (pedscene.h:34-36); velocity persists
        const int k = w.W > 1 ? j / w.Pw : 0;
        double* p = w.sfm.p + 3 * ((size_t)k * w.sfm.n + (size_t)(j - k * w.sfm.n_peds));  // its world's crowd
        p[0] = x;
        p[1] = y;
        p[2] = 0.0;
    }
    w.ped_state[4 * j] = x;
    w.ped_state[4 * j + 1] = y;
    w.ped_state[4 * j + 2] = w.pvx[j];
    w.ped_state[4 * j + 3] = w.pvy[j];
}

// device-side overflow flags (raised by kernels, see world.h / sfm.h): turn them into an error at the next API call
static int check_device_flags(imgenv* h) {
    const volatile int* e = h->err_host;
    if (!e) return 0;
    if (e[0]) FAIL(IMGENV_EDEVICE, "ORCA: a pedestrian sees more obstacle segments than the neighbour scratch holds");
    if (e[1]) FAIL(IMGENV_EDEVICE, "ORCA: obstacle BSP walk overflowed its stack");
    if (e[2])
        FAIL(IMGENV_EDEVICE, "device-side auto-reset: a finished world could not be given its placement (code %d: 100 the pool did not hold it; "
                             "1 a fixed start with a random target; 2-4 no admissible placement within 200000 draws; 10-16 the RVO obstacle tree "
                             "outgrew its scratch)", e[2]);
    if (e[7]) FAIL(IMGENV_EDEVICE, "the observation's gate gave up after 60 s: the caller's stream never reached the step's move (the stream is stuck behind something)");
    if (e[6] == 10) FAIL(IMGENV_EDEVICE, "class layer (counts) in a robot shard: a footprint cell fell outside the record's bitmap (internal)");
    if (e[6] == 9)
        FAIL(IMGENV_EDEVICE, "class layer (counts): more robot footprints on one cell than the layer's count field holds (at least 63; robots "
                             "were placed on top of each other) -- create the handle with IMGENV_FLAG_COMPOSE_DENSE, whose owner layers have no such limit");
    if (e[6]) FAIL(IMGENV_EDEVICE, "class layer (counts): a pedestrian's footprint left its raster box or its cell list (code %d)", e[6]);
    if (e[4])
        FAIL(IMGENV_EDEVICE, "pedscene: the social-force quadtree overflowed (code %d: 1 leaf capacity, 2 node pool, 3 / 4 depth, 5 a leaf lock never came free, "
                             "6 an agent a split re-homed is on the other side of its new leaf's edge than its own move assumed) -- more than "
                             "8 agents piled up outside the tree's 10 m x 10 m root square, where the reference recurses forever "
                             "(ped_tree.cpp:65-96)", e[4]);
    return 0;
}

// what the tails need, whichever kernel ends up running them (tail_group)
static void set_tail_fields(imgenv* h, int is_reset, int tail_elapsed) {
    DevWorld& d = h->d;
    d.tail_fused = h->P > 0 ? 1 : 0;
    d.tail_is_reset = is_reset;
    d.tail_elapsed = tail_elapsed;
}

// The fused tails (tail_group in kernels.h) rely on tail_sig / tail_cnt being zero when a chain of launches starts; the chain
// itself re-zeroes them.  A chain that was abandoned half-way (an error between imgenv_step_begin and imgenv_step_end, a failing
// launch) leaves stale bits behind: the next chain clears the words first.
static int chain_begin(imgenv* h, hipStream_t st) {
    if (h->step.chain_open) {
        HIPCHK(hipMemsetAsync(h->d.tail_sig, 0, sizeof(unsigned long long) * (size_t)h->RL, st));
        HIPCHK(hipMemsetAsync(h->d.tail_cnt, 0, sizeof(int) * (size_t)(h->RL + WAVE - 1) / WAVE * TAIL_CNT_STRIDE, st));
    }
    h->step.chain_open = true;
    return 0;
}

// ---- output guards.  The arrays behind imgenv_outputs() are the kernels' incremental working copies (a step rewrites what can
// change), so a caller that writes into them -- an in-place normalisation in a trainer -- would corrupt every later observation
// silently, where the reference hands out fresh copies (ROS responses, img_env.cpp:745-749).  Two opt-in answers:
// IMGENV_FLAG_CHECK_OUTPUTS seals every array with a checksum at the end of a chain of launches and verifies it at the start
// of the next call (debug: it synchronises); IMGENV_FLAG_FULL_REWRITE hands out a second arena that receives a complete copy
// of every array at the end of every chain, so nothing the caller does to it can reach the kernels.
static int outputs_seal(imgenv* h, hipStream_t st) {
    if (h->pub_arena) HIPCHK(hipMemcpyAsync(h->pub_arena, h->arena, h->arena_bytes, hipMemcpyDeviceToDevice, st));
    if (h->guard_check) {
        HIPCHK(hipMemsetAsync(h->d_sums, 0, sizeof(unsigned long long) * (size_t)h->n_spans, st));
        k_out_sum<<<dim3(h->span_blocks), dim3(256), 0, st>>>(h->d_spans, h->n_spans, h->d_sums);
        h->guard_sealed = true;
    }
    return 0;
}
static int outputs_verify(imgenv* h, hipStream_t st) {
    if (!h->guard_check || !h->guard_sealed) return 0;
    unsigned long long* found = h->d_sums + h->n_spans;
    HIPCHK(hipMemsetAsync(found, 0, sizeof(unsigned long long) * (size_t)h->n_spans, st));
    k_out_sum<<<dim3(h->span_blocks), dim3(256), 0, st>>>(h->d_spans, h->n_spans, found);
    k_out_verify<<<dim3(1), dim3(64), 0, st>>>(h->d_sums, found, h->n_spans, h->d.err);
    HIPCHK(hipStreamSynchronize(st));
    const int f = h->err_host ? h->err_host[5] : 0;
    if (h->guard_left > 0 && --h->guard_left == 0) {  // (IMGENV_FLAG_CHECK_OUTPUTS_FIRST: this was the last look)
        h->guard_check = false;
        h->guard_sealed = false;
    }
    if (f) {
        h->err_host[5] = 0;
        h->guard_sealed = false;  // (the next chain seals what it finds; the caller has been told)
        FAIL(IMGENV_EINVAL, "the caller wrote into imgenv_out.%s since the last call: the output arrays are the library's working copies "
                            "and read-only (include/imgenv.h); create the handle with IMGENV_FLAG_FULL_REWRITE to receive copies instead",
             h->span_name[f - 1]);
    }
    return 0;
}

// Recovery from a step that was begun and never ended (the caller's exchange failed in between), at the reset that follows: its
// k_obs is in flight on a side stream and will still arrive at the tails' hand-over words; wait for it, the reset's first chain
// then clears them (StepState::chain_open is still set).  Nothing else of StepState is touched.
static int step_recover(imgenv* h) {
    if (!h->step.obs_forked) return 0;
    if (h->side2) HIPCHK(hipStreamSynchronize(h->side2));
    h->step.obs_forked = false;
    return 0;
}

static int launch_obs_kernel(imgenv* h, hipStream_t s_obs, bool early_step = false) {
    DevWorld& d = h->d;
    const LaunchShape o = plan_obs(h->plan, chain_facts(h, 0), early_step);
    TIMED(h, IMGENV_K_OBS, s_obs, (k_obs_for(h->plan)<<<dim3(o.grid), dim3(o.block), o.lds, s_obs>>>(d, h->PP)));
    h->launches += 1;
    return 0;
}

static int launch_obs(imgenv* h, hipStream_t st) {
    if (int rc = chain_begin(h, st)) return rc;
    const bool overlap = !h->serial;
    hipStream_t s_obs = overlap ? h->side2 : st;
    if (overlap) {
        if (!h->step.fork_on_move) HIPCHK(hipEventRecord(h->ev_fork, st));
        h->step.fork_on_move = false;
        HIPCHK(hipStreamWaitEvent(s_obs, h->ev_fork, 0));
    }
    if (int rc = launch_obs_kernel(h, s_obs)) return rc;
    h->step.obs_forked = true;
    return 0;
}

// The rasters of a chain of launches, as plan_rasters shapes them (in front of them, in STAMP mode, every STAMP_TAGS steps the sweep)
static int launch_rasters(imgenv* h, hipStream_t st, int is_reset, bool moved, bool local_only, bool from_begin = false) {
    DevWorld& d = h->d;
    const PlanHandle& p = h->plan;
    const PlanChain c = chain_facts(h, is_reset, moved, local_only);
    if (const RasterPackPlan k = plan_raster_pack(p, c); k.rpw) {  // (the id and name stay k_raster's: bench.py --full prices kernels by them)
        TIMED(h, IMGENV_K_RASTER, st, (k_raster_pack_for(p, k.rpw)<<<dim3(k.launch.grid), dim3(k.launch.block), k.launch.lds, st>>>(d)));
        return 0;
    }
    const RasterPlan r = plan_rasters(p, c);
    const int keep_ng = d.act_ng;
    if (local_only) {
        d.act_ng = h->RL;
        d.act_g0 = h->r0;
    }
    if (r.sweep) TIMED(h, IMGENV_K_COMPOSE, st, (k_cell_base<<<dim3(r.sweep_blocks), dim3(256), 0, st>>>(d)));
    const dim3 gr(r.launch.grid), br(r.launch.block);
    // (imgenv_step_end has counted the step when it launches this; imgenv_step_begin has not yet)
    const int step_now = from_begin ? h->elapsed : h->elapsed - 1;
    if (r.move)
        TIMED(h, IMGENV_K_MOVE_RASTER, st, (k_move_raster_for(p, r.nw)<<<gr, br, r.launch.lds, st>>>(d, h->step.actions, h->n_sub, step_now, r.move_peds)));
    else
        TIMED(h, IMGENV_K_RASTER, st, (k_raster_for(p, r.nw)<<<gr, br, r.launch.lds, st>>>(d, is_reset, r.split)));
    d.act_ng = keep_ng;
    d.act_g0 = 0;
    return 0;
}

// The robot rows the chain in hand covers, for its tail kernels (tail_rows.h): every local one, or those of a reset chain's list
static TailRows tail_rows(const imgenv* h, int is_reset) {
    const DevWorld& d = h->d;
    return {h->RL, h->Rw, is_reset ? d.act_list : nullptr, is_reset ? d.act_n_dev : nullptr, d.act_nw};
}

// A step on a handle whose rollout storage holds its whole horizon: refused by every step entry point before it queues anything
static int rollout_room(const imgenv* h) {
    if (h->roll.on && h->roll.begun && h->roll.n >= h->roll.cfg.horizon)
        FAIL(IMGENV_EINVAL, "rollout full: imgenv_rollout_begin (all %d transitions of the horizon are stored)", h->roll.cfg.horizon);
    return 0;
}

// ---- the chain behind the move (launch_views): what its phases share -- the chain's facts and plans, made once
struct ChainPlans {
    int is_reset;
    bool moved;  // the move was left to this chain's raster launch (k_move_raster)
    PlanChain c;
    SidePlan s;
    SideWiring w;
    ViewPlan v;
};
static hipStream_t stream_of(const imgenv* h, int on, hipStream_t st) { return on == ON_SIDE ? h->side : on == ON_SIDE2 ? h->side2 : st; }
template <typename T>
static T* snap_buf(T* (&buf)[2], int k) { return k < 0 ? nullptr : buf[k]; }
// rasters, compose and view count as three launches whatever the layer mode and the view's kind make of them: imgenv_step_launches
// is compared between handles as it is
static constexpr int CHAIN_FIXED_LAUNCHES = 3;

// 1. The final observations (final_obs.h), in front of everything of this chain that writes a captured field -- its k_obs (forked
// behind this launch in stream order), its views and their tails, its k_stack<true> and k_obs_post<true>: the rows the chain
// covers, as the last step left them.  What a reset chain has launched before this point (the staged copies and map restores,
// k_respawn and the rest of the device-side reset) writes none of them.
static int launch_final_obs(imgenv* h, hipStream_t st) {
    FinalObsDev fo = h->final_obs.dev;
    fo.rows = tail_rows(h, 1);
    const PlanChain cf = chain_facts(h, 1);
    const int guess = cf.n_dev ? plan_dev_reset(h->plan, h->finished_host[0], 0).guess : 0;
    const LaunchShape g = plan_final_obs_launch(h->plan, cf, fo.chunks_per_row, guess);
    k_final_obs<<<dim3(g.grid), dim3(g.block), 0, st>>>(fo);
    h->launches += 1;
    return 0;
}

// 2. A robot shard in SUM mode has drawn its own robots in imgenv_step_begin, in front of the exchange, and takes the other ranks'
// from their records now, right behind it; "the records are complete" for the side streams rides on this kernel's dispatch packet
// (a hipEventRecord behind the exchange is a packet of its own on the caller's stream: ~6 us)
static int launch_remote(imgenv* h, hipStream_t st, const ChainPlans& k) {
    const hipEvent_t ev = k.w.fork2_on_remote ? h->ev_fork2 : nullptr;
    TIMED(h, IMGENV_K_REMOTE, st, (hipExtLaunchKernelGGL(k_remote_for(h->plan), dim3(k.s.remote.grid), dim3(k.s.remote.block), 0, st, nullptr, ev, 0, h->d)));
    h->launches += 1;
    return 0;
}

// 3. Beside the rasters, compose and view run the pedestrian half of the observation (unless it went out with the step) and the
// next step's _step_ped_normal solve (img_env.cpp:304-343), on the streams and behind the events plan_side_wiring names; both
// need poses only.
static int launch_side(imgenv* h, hipStream_t st, const ChainPlans& k) {
    DevWorld& d = h->d;
    const SidePlan& s = k.s;
    const SideWiring& w = k.w;
    hipStream_t s_orca = stream_of(h, w.solve_on, st), s_obs = stream_of(h, w.obs_on, st);
    if (!h->step.obs_forked) RTRY(launch_obs(h, st));
    h->step.obs_forked = false;
    if (w.record_fork2) HIPCHK(hipEventRecord(h->ev_fork2, st));
    if (w.solve_waits) HIPCHK(hipStreamWaitEvent(s_orca, w.solve_waits == WAIT_FORK2 ? h->ev_fork2 : h->ev_fork, 0));
    if (!s.fold_side) {
        k_side_robots<<<dim3(s.robots.grid), dim3(s.robots.block), 0, s_orca>>>(d, k.is_reset, s.rvo_agents, s.slices);
        h->launches += 1;
    }
    if (s.orca) {
        const SnapTurn t = plan_snap_turn(h->step.orca_seq, h->early, k.c.listed);
        d.ped_snap_out = snap_buf(h->ped_snap, t.out);
        d.ped_snap_out2 = snap_buf(h->ped_snap, t.out2);
        TIMED(h, IMGENV_K_ORCA, s_orca, (k_orca<<<dim3(s.orca_blocks), dim3(WAVE), orca_lds_bytes(s.L), s_orca>>>(d, s.L)));
        if (t.advance) h->step.orca_seq += 1;
        h->launches += 1;
    }
    if (w.join) {
        HIPCHK(hipEventRecord(h->ev_join, s_orca));
        HIPCHK(hipStreamWaitEvent(s_obs, h->ev_join, 0));
    }
    if (w.join2) HIPCHK(hipEventRecord(h->ev_join2, s_obs));
    return 0;
}

// 6. Compose, then the views: view_big.h's crop -> beams -> the shrunk sensor_map -> the full view, only where it is an output --
// or k_view, which also leaves the snapshot the next early k_obs reads.  No launch for the per-robot scalars: the k_view / k_obs
// wavefront that completes a group of 64 robots runs them (tail_group); the last kernel commits the robots' new is_collision_.
static int launch_compose_views(imgenv* h, hipStream_t st, const ChainPlans& k) {
    DevWorld& d = h->d;
    const PlanHandle& p = h->plan;
    const ViewPlan& v = k.v;
    if (p.layer == LAYER_COMPOSED) TIMED(h, IMGENV_K_COMPOSE, st, (k_compose<<<dim3(plan_compose_blocks(p, k.c)), dim3(256), 0, st>>>(d)));
    if (!p.big_view) {
        const SnapTurn t = plan_snap_turn(h->step.view_seq, h->early, k.c.listed);
        d.rec_snap_out = snap_buf(h->rec_snap, t.out);
        d.rec_snap_out2 = snap_buf(h->rec_snap, t.out2);
        if (t.advance) h->step.view_seq += 1;
        TIMED(h, IMGENV_K_VIEW, st, (hipExtLaunchKernelGGL(k_view_for(p, v.nw), dim3(v.view.grid), dim3(v.view.block), (uint32_t)v.view.lds, st, nullptr, nullptr, 0, d)));
        return 0;
    }
    TIMED(h, IMGENV_K_CROP, st, (k_crop_big_for(v.crop_sel)<<<dim3(v.crop.grid), dim3(v.crop.block), 0, st>>>(d, v.crop_chunks, k.c.act_nl, v.tpw)));
    TIMED(h, IMGENV_K_VIEW, st, (k_beams_big_for(p)<<<dim3(v.beams.grid), dim3(v.beams.block), v.beams.lds, st>>>(d, v.quarters, v.qpw)));
    if (v.taps)
        TIMED(h, IMGENV_K_TAPS, st, (k_taps_big<<<dim3(v.taps_shape.grid), dim3(v.taps_shape.block), v.taps_shape.lds, st>>>(d, v.tap_wgs, v.full ? 0 : 1, v.listed ? 1 : 0)));
    if (v.full)
        TIMED(h, IMGENV_K_FULLVIEW, st, (k_fullview_big<<<dim3(v.fullview.grid), dim3(v.fullview.block), v.fullview.lds, st>>>(d, h->big_full_chunks, 1)));
    h->launches += (v.taps ? 1 : 0) + (v.full ? 1 : 0);
    return 0;
}

// 8. The tails of the optional features, on the caller's stream behind the join of the side streams and in front of the seal; each
// is a no-op unless its feature is on, and stands with its feature's enable function.  A step covers every local robot, a reset
// chain the robots of its list (tail_rows).  The order is who reads whose output: the stacks push the chain's new frames; the
// episode log reads the state the episodes' fold then closes; obs_post behind them (k_stack<true>'s cases); the normalisation
// reads the stacks' newest frames; the rollout storage, last, stores what k_stack, k_obs_post and the normalisation have written.
static void tail_stack(imgenv* h, hipStream_t st, const ChainPlans& k);
static void tail_episodes(imgenv* h, hipStream_t st, const ChainPlans& k);
static void tail_obs_post(imgenv* h, hipStream_t st, const ChainPlans& k);
static void tail_normalise(imgenv* h, hipStream_t st, const ChainPlans& k);
static void tail_rollout(imgenv* h, hipStream_t st, const ChainPlans& k);
static void launch_tails(imgenv* h, hipStream_t st, const ChainPlans& k) {
    tail_stack(h, st, k);
    tail_episodes(h, st, k);
    tail_obs_post(h, st, k);
    tail_normalise(h, st, k);
    tail_rollout(h, st, k);
}

// The chain behind the move -- plan, then launch in stream order.  The rasters come first in a step whose move was left to them
// (imgenv_step_begin: k_move_raster; the side stream forks behind them), otherwise behind the side launches; k_remote has drawn a
// SUM shard's.
static int launch_views(imgenv* h, hipStream_t st, int is_reset) {
    set_tail_fields(h, is_reset, h->elapsed);
    if (is_reset && h->final_obs.on && h->step.obs_exists) RTRY(launch_final_obs(h, st));
    if (h->P == 0) RTRY(chain_begin(h, st));
    ChainPlans k;
    k.is_reset = is_reset;
    k.moved = h->step.move_pending;
    h->step.move_pending = false;
    k.c = chain_facts(h, is_reset, k.moved);
    k.s = plan_side(h->plan, k.c);
    k.w = plan_side_wiring(k.s, h->plan, h->step.early);
    k.v = plan_views(h->plan, k.c);
    const bool rasters = !k.s.remote_only;
    if (k.s.remote_only) RTRY(launch_remote(h, st, k));
    if (rasters && k.moved) RTRY(launch_rasters(h, st, is_reset, true, false));
    if (h->P > 0) RTRY(launch_side(h, st, k));
    if (k.s.state) {  // 4. no side streams: after a reset Agent::get_state gets its own small launch
        k_state<<<dim3(k.s.state_shape.grid), dim3(k.s.state_shape.block), 0, st>>>(h->d);
        h->launches += 1;
    }
    if (rasters && !k.moved) RTRY(launch_rasters(h, st, is_reset, false, false));
    RTRY(launch_compose_views(h, st, k));
    h->step.early = false;
    if (k.w.join2) HIPCHK(hipStreamWaitEvent(st, h->ev_join2, 0));  // 7. the caller's stream ends the chain behind both side streams
    h->launches += CHAIN_FIXED_LAUNCHES;
    launch_tails(h, st, k);
    HIPCHK(hipGetLastError());  // 9. finish and seal
    h->step.chain_open = false;
    h->step.obs_exists = true;
    h->step.chain_seq += 1;
    return outputs_seal(h, st);
}

// ---- pinned staging for reset: everything a reset uploads goes through page-locked chunks owned by the handle and
// reaches the device in ONE launch (a table of segments: StageSeg, reset_plan.h), however many worlds the reset covers ----
// a kernel pulls the bytes out of the page-locked chunks: unlike hipMemcpyAsync (which was seen to block the host for
// several milliseconds on a busy stream once a copy exceeds a few hundred KB) a launch never waits
__device__ __forceinline__ void copy_segment(const StageSeg g, size_t t, size_t stride) {
    if ((((uintptr_t)g.dst | (uintptr_t)g.src) & 15) == 0) {
        const size_t n16 = g.bytes / 16;
        for (size_t q = t; q < n16; q += stride) ((uint4*)g.dst)[q] = ((const uint4*)g.src)[q];
        for (size_t q = n16 * 16 + t; q < g.bytes; q += stride) g.dst[q] = g.src[q];
    } else if ((((uintptr_t)g.dst | (uintptr_t)g.src | g.bytes) & 3) == 0) {
        for (size_t q = t; q < g.bytes / 4; q += stride) ((uint32_t*)g.dst)[q] = ((const uint32_t*)g.src)[q];
    } else {
        for (size_t q = t; q < g.bytes; q += stride) g.dst[q] = g.src[q];
    }
}

// Everything of a reset that only depends on the staged bytes, in ONE launch (each dependent launch of the reset chain
// costs the stream ~10 us, whatever its size).  Workgroups, in order:
//   n_seg * per_seg : the segment copies (trajectories, RVO polygons, per-world tables, the world list)
//   n_worlds * MAP_BLOCKS : obs_map_ of each world being reset starts from the static map again (img_env.cpp:166-168)
//   robots, pedestrians : init_pose / set_goal / setPedPos ..., straight from the page-locked host blocks
struct ResetArgs {
    const StageSeg* table;
    int n_seg, per_seg;
    const int* list;  // the worlds of this reset (page-locked host copy), nullptr = every world
    int n_worlds;
    const uint8_t* static_map;
    const double* rob3;
    const ResetRobot* rr;
    const double* ped3;
    int n_robots, n_peds, whole;
    int stamp;  // STAMP mode: the class layer gets its base classes here too (k_reset_obstacles keeps it in step)
    MapSel maps;  // map bank: which map of static_map[n_maps][stride] each world starts from (csrc/map_bank.h)
};
static int stage_begin(imgenv* h) {
    imgenv::ResetStage& s = h->rs;
    s.gen = (s.gen + 1) % imgenv::STAGE_GENS;
    const int g = s.gen;
    if (!s.ev_gen[g]) HIPCHK(hipEventCreateWithFlags(&s.ev_gen[g], hipEventDisableTiming));
    if (s.gen_pending[g]) {  // the copies of the reset STAGE_GENS calls ago (long finished in practice) still own these chunks
        HIPCHK(hipEventSynchronize(s.ev_gen[g]));
        s.gen_pending[g] = false;
    }
    for (auto& c : s.chunks[g]) c.used = 0;
    s.segs.clear();
    s.seg_max = 0;
    return 0;
}
static int stage_room(imgenv* h, size_t bytes, unsigned char** out) {
    imgenv::Chunk* use = nullptr;
    std::vector<imgenv::Chunk>& chunks = h->rs.chunks[h->rs.gen];
    for (auto& c : chunks)
        if (c.cap - c.used >= bytes) {
            use = &c;
            break;
        }
    if (!use) {
        imgenv::Chunk c{nullptr, std::max(bytes, (size_t)1 << 20), 0};
        HIPCHK(hipHostMalloc((void**)&c.p, c.cap, hipHostMallocDefault));
        chunks.push_back(c);
        use = &chunks.back();
    }
    *out = use->p + use->used;
    use->used += (bytes + 255) & ~(size_t)255;
    if (use->used > use->cap) use->used = use->cap;
    return 0;
}
// page-locked room for n elements that k_reset_apply copies to dst; the caller fills *out
template <typename T>
static int stage_seg(imgenv* h, T* dst, size_t n, T** out) {
    unsigned char* p = nullptr;
    if (int rc = stage_room(h, sizeof(T) * n, &p)) return rc;
    *out = (T*)p;
    if (n == 0) return 0;
    h->rs.segs.push_back(StageSeg{(unsigned char*)dst, p, sizeof(T) * n});
    h->rs.seg_max = std::max(h->rs.seg_max, sizeof(T) * n);
    return 0;
}
template <typename T, typename S>
static int stage_put(imgenv* h, T* dst, const S* src, size_t bytes) {
    if (bytes == 0) return 0;
    unsigned char* p = nullptr;
    if (int rc = stage_seg(h, (unsigned char*)dst, bytes, &p)) return rc;
    memcpy(p, src, bytes);
    return 0;
}
// n ints in page-locked room of their own, for a kernel to read in place
static int stage_ints(imgenv* h, const int* src, size_t n, int** out) {
    unsigned char* p = nullptr;
    if (int rc = stage_room(h, sizeof(int) * n, &p)) return rc;
    memcpy(p, src, sizeof(int) * n);
    *out = (int*)p;
    return 0;
}
static int stage_end(imgenv* h, hipStream_t st) {
    HIPCHK(hipEventRecord(h->rs.ev_gen[h->rs.gen], st));
    h->rs.gen_pending[h->rs.gen] = true;
    return 0;
}

// a launch covers every world (list == nullptr) or the robots, pedestrians and cells of the n listed worlds
static void set_active(imgenv* h, const int* list, int n) {
    DevWorld& d = h->d;
    d.act_cells = h->W > 1 ? h->Gs * h->W : h->Gs;
    if (!list) {
        d.act_list = nullptr; d.act_nw = h->W; d.act_nl = h->RL; d.act_ng = h->R; d.act_np = h->P;
    } else {
        d.act_list = list; d.act_nw = n; d.act_nl = d.act_ng = n * h->Rw; d.act_np = n * h->Pw;
    }
}

__global__ void k_restride3(double* __restrict__ dst, const double* __restrict__ src, int n, int old_cap, int new_cap) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)n * old_cap * 3) return;
    const size_t j = t / ((size_t)old_cap * 3), rem = t - j * (size_t)old_cap * 3;
    dst[j * (size_t)new_cap * 3 + rem] = src[t];
}

__global__ __launch_bounds__(256) void k_reset_apply(DevWorld w, ResetArgs a) {
    int b = blockIdx.x;
    if (b < a.n_seg * a.per_seg) {
        copy_segment(a.table[b / a.per_seg], (size_t)(b % a.per_seg) * blockDim.x + threadIdx.x, (size_t)a.per_seg * blockDim.x);
        return;
    }
    b -= a.n_seg * a.per_seg;
    if (b < a.n_worlds * MAP_BLOCKS) {
        const int q = b / MAP_BLOCKS, world = a.list ? a.list[q] : q;
        const size_t n16 = ((size_t)w.Hg * w.Wg + 15) / 16;  // (both buffers are padded to 16 bytes)
        int map_id = 0;
        if (a.maps.cur) {  // the world's map of the bank: what imgenv_world_maps_set chose, or the host's draw for this placement
            map_id = a.maps.ids ? a.maps.ids[q] : a.maps.next[world];
            if (b == q * MAP_BLOCKS && threadIdx.x == 0) {  // (no block of this launch reads what this writes)
                a.maps.cur[world] = map_id;
                if (a.maps.ids) a.maps.next[world] = map_id;
            }
        }
        const uint4* bank = (const uint4*)(a.static_map + (size_t)map_id * a.maps.stride);
        uint4* dst = (uint4*)(const_cast<uint8_t*>(w.obs_map) + (size_t)world * w.Gs);
        uint4* cls = (uint4*)(w.cell + (size_t)world * w.Gs);
        for (size_t e = (size_t)(b - q * MAP_BLOCKS) * blockDim.x + threadIdx.x; e < n16; e += (size_t)MAP_BLOCKS * blockDim.x) {
            const uint4 v = bank[e];
            dst[e] = v;
            if (a.stamp) {  // base class of 16 cells, no stamp (2, SUM mode: the counts on the cells stay -- their owners take them off)
                const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    uint32_t c4[4];
                    const uint4 old = a.stamp == 2 ? cls[4 * e + k] : make_uint4(0, 0, 0, 0);
                    const uint32_t keep[4] = {old.x & ~7u, old.y & ~7u, old.z & ~7u, old.w & ~7u};
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const uint32_t o = (wd[k] >> (8 * j)) & 0xFFu;
                        c4[j] = (o <= 2 ? o : (o < 250 ? CLS_LOW : CLS_HIGH)) | keep[j];
                    }
                    cls[4 * e + k] = make_uint4(c4[0], c4[1], c4[2], c4[3]);
                }
            }
        }
        if (w.crop_map) {  // view_big.h's one-byte-per-cell summary of the map starts over with it
            const uint4* src = (const uint4*)(w.static_crop + (size_t)map_id * w.crop_ws);
            uint4* cm = (uint4*)(w.crop_map + (size_t)world * w.crop_ws);
            for (size_t e = (size_t)(b - q * MAP_BLOCKS) * blockDim.x + threadIdx.x; e < w.crop_ws / 16; e += (size_t)MAP_BLOCKS * blockDim.x) cm[e] = src[e];
        }
        return;
    }
    b -= a.n_worlds * MAP_BLOCKS;
    const int robot_blocks = (a.n_robots + 255) / 256;
    if (b < robot_blocks) {
        const int t = b * 256 + threadIdx.x;
        if (t < a.n_robots) reset_robot(w, a.list, t, a.rob3, a.rr, a.whole);
        return;
    }
    const int t = (b - robot_blocks) * 256 + threadIdx.x;
    if (t < a.n_peds) reset_ped(w, a.list, t, a.ped3);
}
// Every obstacle is then drawn into its world's map with value 0: Agent::draw(obs_map, 0, "world_map") (img_env.cpp:169-193,
// agent.cpp:285-327) writes unless the cell holds 0 / 1 / 2 -- and only ever writes 0, so the order does not matter.
// One workgroup per obstacle.  Its footprint samples (agent.cpp:18-30, 51-62: a 0.01 m lattice, for circles the points within
// the radius) are generated on the fly from the lattice bounds the host computed: random obstacle radii (EnvPos draws a fresh
// one per episode, reset_helper.py:131-133) then cost nothing -- no per-size sample list to upload, cache or free (ObstInst, reset_plan.h).
template <bool POW2>
__global__ __launch_bounds__(256) void k_reset_obstacles(DevWorld w, const ObstInst* __restrict__ inst, int stamp, const int* n_dev, int per_world, int parts,
                                                        ObstInst* keep, int* keep_valid) {
    // parts workgroups share an obstacle's samples (a reset of a few worlds is a handful of obstacles: their latency is the launch's)
    const int t0 = (int)blockIdx.x / parts, part = (int)blockIdx.x - t0 * parts;
    // device-side auto-reset: per_world instances for each finished world, the grid sized for a guess of their number
    for (int t = t0; t < (n_dev ? *n_dev * per_world : t0 + 1); t += (int)gridDim.x / parts) {
        const ObstInst o = inst[t];
        if (o.world < 0) continue;  // (a finished world whose placement failed: k_respawn)
        if (keep && part == 0 && threadIdx.x == 0) {  // ... which remembers what each world now carries, for the next restore (k_restore_maps_dev)
            keep[(size_t)o.world * per_world + (t % per_world)] = o;
            keep_valid[o.world] = 1;
        }
        const Tf2 bw = tf_from_pose_sc(o.x, o.y, o.sh, o.ch);
        uint8_t* map = const_cast<uint8_t*>(w.obs_map) + (size_t)o.world * w.Gs;
        const double resolution = 0.01;
        const int nn = o.n1 - o.n0 + 1, total = (o.m1 - o.m0 + 1) * nn;
        const bool circle = o.shape == IMGENV_SHAPE_CIRCLE;
        for (int q = part * (int)blockDim.x + (int)threadIdx.x; q < total; q += parts * (int)blockDim.x) {
            const int m = o.m0 + q / nn, n = o.n0 + q % nn;
            double px = m * resolution, py = n * resolution;
            if (circle) {
                if (!(sqrt(m * resolution * m * resolution + n * resolution * n * resolution) <= o.r)) continue;
                px = px + o.cx;
                py = py + o.cy;
            }
            double wx, wy;
            tf_apply(bw, px, py, wx, wy);
            int gm, gn;
            w2m_pair<POW2>(wx, wy, w.res, w.inv_res, gm, gn);
            if (gm >= 0 && gm < w.Hg && gn >= 0 && gn < w.Wg) {
                const size_t at = (size_t)gm * w.Wg + gn;
                if (map[at] > 2) {
                    map[at] = 0;
                    if (stamp == 1) w.cell[(size_t)o.world * w.Gs + at] = CLS_STATIC;  // the class layer's base class follows
                    else if (stamp == 2) w.cell[(size_t)o.world * w.Gs + at] &= ~7u;        // (SUM mode: the counts stay; every writer of this cell writes the same word)
                    if (w.crop_map) w.crop_map[(size_t)o.world * w.crop_ws + crop_tiled(w, (uint32_t)gm, (uint32_t)gn)] = 0;  // ... and view_big.h's byte: not free, no stamp
                }
            }
        }
    }
}

#include "spawn_device.h"  // device-side auto-reset: k_spawn_fill, k_finished_dev, k_respawn, k_restore_maps_dev
#include "track_bank.h"    // recorded crowds: k_tracks_install
#include "scenario_bank.h"  // recorded episodes: k_scenario_fill

static auto k_reset_obstacles_for(const PlanHandle& p) { return p.pow2 ? k_reset_obstacles<true> : k_reset_obstacles<false>; }
static auto k_restore_maps_dev_for(const PlanHandle& p) { return p.pow2 ? k_restore_maps_dev<true> : k_restore_maps_dev<false>; }

static MapSel map_sel(const imgenv* h) {
    MapSel m;
    m.cur = h->d_map_cur; m.next = h->d_map_next; m.ids = nullptr;
    m.stride = h->map_stride; m.n_maps = h->n_maps;
    m.by_placement = h->maps_policy == IMGENV_MAPS_BY_PLACEMENT && h->n_maps > 1 ? 1 : 0;
    return m;
}

static TrackSel track_sel(const imgenv* h) {
    TrackSel t;
    t.traj = h->d_trk_traj; t.traj_v = h->d_trk_traj_v; t.pose3 = h->d_trk_pose3; t.len = h->d_trk_len;
    t.cur = h->d_trk_cur; t.next = h->d_trk_next; t.count = h->d_trk_count;
    t.n_sets = h->n_track_sets; t.cap = h->trk_cap;
    t.policy = h->tracks_policy; t.repeat = h->tracks_repeat;
    return t;
}

// ---- a host-side reset: prepare (reset_plan.h: what every listed world's batch brings, nothing of the handle written), refuse
// (every refusal of the path, before the handle or the device is touched), commit (grow once, stage every destination once, launch)
static ResetFacts reset_facts(const imgenv* h) {
    ResetFacts f;
    f.W = h->W; f.Rw = h->Rw; f.Pw = h->Pw; f.r0 = h->r0; f.RL = h->RL; f.NA = h->NA;
    f.scene = h->cfg.ped_scene_type;
    f.track_bank = h->d_trk_cur != nullptr;
    f.dev_reset_used = h->dev.used;
    f.cap_obst = h->cap_obst; f.cap_nodes = h->cap_nodes; f.sfm_cap_obs = h->sfm_cap_obs; f.traj_cap = h->traj_cap;
    f.sfm_n = h->d.sfm.n; f.sfm_per_world = h->d.sfm.n_obs_w != nullptr; f.has_traj = h->d_traj != nullptr;
    return f;
}
// world k's share of a whole-handle batch: its robots and pedestrians (world-major numbering), one obstacle list for all
static imgenv_reset_batch world_batch(const imgenv* h, const imgenv_reset_batch* b, int k) {
    imgenv_reset_batch sub = *b;
    sub.robot_pose = b->robot_pose + (size_t)4 * k * h->Rw;
    sub.robot_goal = b->robot_goal + (size_t)2 * k * h->Rw;
    if (h->P > 0) {
        sub.ped_pose = b->ped_pose ? b->ped_pose + (size_t)4 * k * h->Pw : nullptr;  // (null: a bank-fed batch, reset_check_batches)
        sub.ped_goal = b->ped_goal ? b->ped_goal + (size_t)2 * k * h->Pw : nullptr;
        sub.ped_traj_len = b->ped_traj_len ? b->ped_traj_len + (size_t)k * h->Pw : nullptr;
        sub.ped_traj = b->ped_traj ? b->ped_traj + (size_t)k * h->Pw * b->ped_traj_cap * 3 : nullptr;
        sub.ped_traj_v = b->ped_traj_v ? b->ped_traj_v + (size_t)k * h->Pw * b->ped_traj_cap * 2 : nullptr;
    }
    return sub;
}
// prepare + refuse.  worlds == nullptr: every world of the handle from the one batch
static int reset_prepare(imgenv* h, const ResetFacts& f, int n, const int32_t* worlds, const imgenv_reset_batch* batches) {
    h->rs.worlds.resize((size_t)n);
    for (int q = 0; q < n; q++) reset_prepare_world(f, worlds ? worlds[q] : q, batches[worlds ? q : 0], h->rs.worlds[q]);
    return reset_check_worlds(f, h->rs.worlds.data(), n, g_err);
}
// what a reset asks of the handle and the device before it commits
static int reset_device_ready(imgenv* h, hipStream_t st) {
    RTRY(step_recover(h));
    HIPCHK(hipSetDevice(h->cfg.device));
    if (int rc = check_device_flags(h)) {  // report what the abandoned episode raised, then start clean
        for (int q = 0; q < 8; q++) h->err_host[q] = 0;
        return rc;
    }
    if (!h->d_act_list) RTRY(dev_alloc(h, &h->d_act_list, (size_t)h->W));
    return outputs_verify(h, st);
}

// page-locked blocks for the robots / pedestrians of the n worlds of this reset, in list order (read by k_reset_apply)
static int reset_blocks(imgenv* h, int n, const int* list) {
    imgenv::ResetStage& s = h->rs;
    unsigned char* p = nullptr;
    const size_t n_local = h->W > 1 ? (size_t)n * h->Rw : (size_t)h->RL;
    RTRY(stage_room(h, sizeof(double) * 5 * n * h->Rw, &p));
    s.rob3 = (double*)p;
    RTRY(stage_room(h, sizeof(ResetRobot) * std::max<size_t>(n_local, 1), &p));
    s.rr = (ResetRobot*)p;
    RTRY(stage_room(h, sizeof(double) * 3 * std::max<size_t>((size_t)n * h->Pw, 1), &p));
    s.ped3 = (double*)p;
    s.list = nullptr;
    s.fed.clear();
    s.fed_ids.clear();
    if (list) RTRY(stage_ints(h, list, (size_t)n, &s.list));
    return 0;
}

// commit, 1: the tables grow once, before the first segment is queued (reset_growth)
static int reset_grow(imgenv* h, const ResetGrowth& g, hipStream_t st) {
    DevWorld& d = h->d;
    if (g.cap_obst != h->cap_obst) {
        RTRY(dev_alloc(h, &h->d_obst, (size_t)g.cap_obst * h->W));
        h->cap_obst = g.cap_obst;
    }
    if (g.cap_nodes != h->cap_nodes) {
        RTRY(dev_alloc(h, &h->d_nodes, (size_t)g.cap_nodes * h->W));
        h->cap_nodes = g.cap_nodes;
    }
    if (g.sfm_moved) {
        RTRY(dev_alloc(h, &d.sfm.obs, (size_t)g.sfm_cap_obs * 4));
        h->sfm_cap_obs = d.sfm.cap_obs = g.sfm_cap_obs;
    }
    if (g.traj_moved) {  // longer trajectories than any before: the table is laid out again (the worlds not listed keep theirs)
        const bool dataset = h->cfg.ped_scene_type == IMGENV_SCENE_DATASET;
        const int old_cap = h->traj_cap;
        double *old_t = h->d_traj, *old_v = h->d_traj_v;
        RTRY(dev_alloc(h, &h->d_traj, (size_t)h->P * g.traj_cap * 3));
        if (dataset) RTRY(dev_alloc(h, &h->d_traj_v, (size_t)h->P * g.traj_cap * 3));
        h->traj_cap = g.traj_cap;
        if (h->W > 1 && old_cap > 0) {
            const size_t n = (size_t)h->P * old_cap * 3;
            k_restride3<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st>>>(h->d_traj, old_t, h->P, old_cap, h->traj_cap);
            if (dataset) k_restride3<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st>>>(h->d_traj_v, old_v, h->P, old_cap, h->traj_cap);
        }
    }
    return 0;
}
// commit, 2: the prepared obstacle sets become the handle's (swapped, not copied) and the slices of reset_rvo_worlds go up, each once
static int stage_rvo(imgenv* h, const int* list, int n, const ResetGrowth& g) {
    static_assert(sizeof(RvoObstHost) == sizeof(RvoObstDev) && sizeof(RvoNodeHost) == sizeof(RvoNodeDev), "layout");
    for (int q = 0; q < n; q++) std::swap(h->rvos[h->rs.worlds[q].world], h->rs.worlds[q].rvo);
    for (int k : reset_rvo_worlds(h->W, g, list, n)) {
        const RvoObstacles& r = h->rvos[k];
        if (!r.ob.empty()) RTRY(stage_put(h, h->d_obst + (size_t)k * h->cap_obst, r.ob.data(), sizeof(RvoObstDev) * r.ob.size()));
        if (!r.nodes.empty()) RTRY(stage_put(h, h->d_nodes + (size_t)k * h->cap_nodes, r.nodes.data(), sizeof(RvoNodeDev) * r.nodes.size()));
        rvo_table_put(h->wobst, h->W, k, h->cap_obst, h->cap_nodes, r);
    }
    DevWorld& d = h->d;
    d.obst = h->d_obst;
    d.onodes = h->d_nodes;
    d.n_obst = (int)h->rvos[0].ob.size();  // (W > 1: the kernels read the per-world table instead)
    d.n_onodes = (int)h->rvos[0].nodes.size();
    d.oroot = h->rvos[0].root;
    return 0;
}
// commit, 3: one world's rows.  The social-force segments of its crowd ...
static int stage_world_crowd(imgenv* h, const ResetWorld& w) {
    if (h->cfg.ped_scene_type != IMGENV_SCENE_PEDSIM) return 0;
    DevWorld& d = h->d;
    const int k = w.world, nob = (int)w.sfm_obs.size() / 4;
    if (h->W > 1) {  // world k's slice and count
        if (nob) RTRY(stage_put(h, d.sfm.obs + (size_t)k * d.sfm.cap_obs * 4, w.sfm_obs.data(), sizeof(double) * w.sfm_obs.size()));
        h->sfm_nobs_w[k] = nob;
        RTRY(stage_put(h, const_cast<int*>(d.sfm.n_obs_w) + k, &h->sfm_nobs_w[k], sizeof(int)));
    } else {
        if (nob) RTRY(stage_put(h, d.sfm.obs, w.sfm_obs.data(), sizeof(double) * w.sfm_obs.size()));
        d.sfm.n_obs = nob;
    }
    return 0;
}
// ... its pedestrians (img_env.cpp:220-250), written straight into the page-locked rows ...
static int stage_world_peds(imgenv* h, const ResetWorld& w, int q_list, const imgenv_reset_batch* b, const ResetChoices& choices) {
    DevWorld& d = h->d;
    const int k = w.world, Pw = h->Pw, p_lo = k * Pw, cap = h->traj_cap;
    const bool dataset = h->cfg.ped_scene_type == IMGENV_SCENE_DATASET;
    double* ped3 = h->rs.ped3 + (size_t)q_list * Pw * 3;
    if (w.fed) {  // k_tracks_install brings this world's pedestrians (the batch's own pedestrian arrays are ignored)
        h->rs.fed.push_back(k);
        h->rs.fed_ids.push_back(choices.track_ids ? choices.track_ids[q_list] : -1);
        reset_ped_rows(Pw, *b, true, cap, ped3, nullptr, nullptr);
    } else {
        if (dataset && h->d_trk_cur) {  // its own tracks: imgenv_world_tracks says -1, the CYCLE count stays
            static const int minus_one = -1;
            RTRY(stage_put(h, h->d_trk_cur + k, &minus_one, sizeof(int)));
        }
        double* traj = nullptr;
        int* tlen = nullptr;
        RTRY(stage_seg(h, h->d_traj + (size_t)p_lo * cap * 3, (size_t)Pw * cap * 3, &traj));
        RTRY(stage_seg(h, h->d_traj_len + p_lo, (size_t)Pw, &tlen));
        reset_ped_rows(Pw, *b, false, cap, ped3, tlen, traj);
        if (dataset) {
            double* tv = nullptr;
            RTRY(stage_seg(h, h->d_traj_v + (size_t)p_lo * cap * 3, (size_t)Pw * cap * 3, &tv));
            reset_traj_v_rows(Pw, *b, cap, tv);
        }
    }
    if (w.fed || dataset) d.ptraj_v = h->d_traj_v;
    d.ptraj = h->d_traj;
    d.traj_cap = cap;
    return 0;
}
// ... the waypoint deques of a pedscene crowd (this world's pedestrians: the first Pw agents of its crowd) ...
static int stage_world_waypoints(imgenv* h, int k, const imgenv_reset_batch* b) {
    const SfmDev& f = h->d.sfm;
    const size_t a0 = (size_t)k * f.n, n = (size_t)h->Pw * SFM_MAX_WP;  // first agent of world k's crowd
    WaypointRows o;
    RTRY(stage_seg(h, f.wpx + a0 * SFM_MAX_WP, n, &o.wx));
    RTRY(stage_seg(h, f.wpy + a0 * SFM_MAX_WP, n, &o.wy));
    RTRY(stage_seg(h, f.wpr + a0 * SFM_MAX_WP, n, &o.wr));
    RTRY(stage_seg(h, f.dq + a0 * SFM_MAX_WP, n, &o.dq));
    RTRY(stage_seg(h, f.dq_n + a0, (size_t)h->Pw, &o.dq_n));
    RTRY(stage_seg(h, f.dest + a0, (size_t)h->Pw, &o.dest));
    RTRY(stage_seg(h, f.last + a0, (size_t)h->Pw, &o.last));
    reset_waypoint_rows(h->Pw, *b, o);
    return 0;
}
// ... and its robots (img_env.cpp:252-282); `epoch`: h->elapsed at this reset (its TimeLimitWrapper starts over)
static int stage_world(imgenv* h, const ResetFacts& f, const ResetWorld& w, int q_list, const imgenv_reset_batch* b, const ResetChoices& choices, int epoch) {
    RTRY(stage_world_crowd(h, w));
    if (h->Pw > 0) RTRY(stage_world_peds(h, w, q_list, b, choices));
    if (h->Pw > 0 && h->cfg.ped_scene_type == IMGENV_SCENE_PEDSIM) RTRY(stage_world_waypoints(h, w.world, b));
    const size_t n_l = h->W > 1 ? h->Rw : h->RL;  // local robots of this world (a shard exists for W == 1 only)
    reset_robot_rows(f, w.world, *b, h->rs.rob3 + (size_t)q_list * h->Rw * 5, h->rs.rr + (size_t)q_list * n_l);
    h->world_epoch[w.world] = epoch;
    h->world_ready[w.world] = 1;
    return 0;
}

// commit, 4: the small tables of the listed worlds (nullptr: of every world)
static int reset_stage_tables(imgenv* h, const int* list, int n, bool whole_wobst) {
    if (h->dev.ready) {  // a host-side reset draws obstacles the device-side restore does not know: whole-map restore next time
        static const std::vector<int> zeros(1 << 16, 0);
        const SpawnDev& c = h->dev.pool;
        if (!list) {
            for (int k0 = 0; k0 < h->W; k0 += (int)zeros.size())
                RTRY(stage_put(h, c.w_inst_valid + k0, zeros.data(), sizeof(int) * (size_t)std::min<int>((int)zeros.size(), h->W - k0)));
        } else {
            for (int q = 0; q < n; q++) RTRY(stage_put(h, c.w_inst_valid + list[q], zeros.data(), sizeof(int)));
        }
    }
    if (!list || whole_wobst) RTRY(stage_put(h, h->d_wobst, h->wobst.data(), sizeof(int) * h->wobst.size()));  // (every slice moved: the whole table)
    if (!list) {
        RTRY(stage_put(h, h->d_world_epoch, h->world_epoch.data(), sizeof(int) * h->W));
    } else {  // only the listed worlds' entries: the device-side auto-reset keeps the others' up to date itself
        for (int q = 0; q < n; q++) {
            const int k = list[q];
            for (int t = 0; t < 4; t++) RTRY(stage_put(h, h->d_wobst + (size_t)t * h->W + k, &h->wobst[(size_t)t * h->W + k], sizeof(int)));
            RTRY(stage_put(h, h->d_world_epoch + k, &h->world_epoch[k], sizeof(int)));
        }
    }
    if (list) RTRY(stage_put(h, h->d_act_list, list, sizeof(int) * n));  // for the launches after k_reset_apply
    return 0;
}
// the obstacle instances of every prepared world, back to back: one segment
static int reset_stage_obstacles(imgenv* h, int n, size_t* n_inst_out) {
    imgenv::ResetStage& s = h->rs;
    size_t n_inst = 0;
    for (int q = 0; q < n; q++) n_inst += s.worlds[q].inst.size();
    if (n_inst > s.cap_inst) {
        RTRY(dev_alloc(h, &s.d_inst, n_inst * 2));
        s.cap_inst = n_inst * 2;
    }
    ObstInst* at = nullptr;
    if (n_inst) RTRY(stage_seg(h, s.d_inst, n_inst, &at));
    for (int q = 0; q < n && n_inst; at += s.worlds[q].inst.size(), q++) std::copy(s.worlds[q].inst.begin(), s.worlds[q].inst.end(), at);
    *n_inst_out = n_inst;
    return 0;
}
// one launch: segment copies | map restore | robot state | pedestrian state
static int reset_apply(imgenv* h, const ResetPlan& rp, const ResetChoices& choices, hipStream_t st, int whole) {
    imgenv::ResetStage& s = h->rs;
    const DevWorld& d = h->d;
    ResetArgs a;
    unsigned char* table = nullptr;
    RTRY(stage_room(h, std::max<size_t>(s.segs.size(), 1) * sizeof(StageSeg), &table));
    memcpy(table, s.segs.data(), s.segs.size() * sizeof(StageSeg));
    a.table = (const StageSeg*)table;
    a.n_seg = (int)s.segs.size();
    a.per_seg = rp.per_seg;
    a.list = s.list;
    a.n_worlds = d.act_nw;
    a.static_map = h->d_static_map;
    a.maps = map_sel(h);
    if (h->d_map_cur && choices.map_ids) {
        int* ids = nullptr;
        RTRY(stage_ints(h, choices.map_ids, (size_t)d.act_nw, &ids));
        a.maps.ids = ids;
    }
    a.rob3 = s.rob3;
    a.rr = s.rr;
    a.ped3 = s.ped3;
    a.n_robots = d.act_ng;
    a.n_peds = d.act_np;
    a.whole = whole;
    a.stamp = h->plan.layer;
    k_reset_apply<<<dim3(rp.apply.grid), dim3(rp.apply.block), 0, st>>>(d, a);
    s.segs.clear();
    s.seg_max = 0;
    return 0;
}
// the worlds whose batch brought no tracks take their set of the bank: behind the staged copies, in front of the rasters
static int reset_tracks(imgenv* h, hipStream_t st) {
    imgenv::ResetStage& s = h->rs;
    const int n_fed = (int)s.fed.size();
    s.fed.insert(s.fed.end(), s.fed_ids.begin(), s.fed_ids.end());  // [worlds | ids]
    int* fed_list = nullptr;
    RTRY(stage_ints(h, s.fed.data(), s.fed.size(), &fed_list));
    const TracksPlan tp = plan_tracks_install(h->plan, n_fed, false, 0, h->trk_cap);
    k_tracks_install<<<dim3(tp.install.grid), dim3(tp.install.block), 0, st>>>(h->d, track_sel(h), fed_list, nullptr, n_fed, fed_list + n_fed, nullptr, nullptr,
                                                                             0ull, h->d_traj, h->d_traj_v, h->d_traj_len, h->traj_cap);
    s.fed.clear();
    s.fed_ids.clear();
    return 0;
}
// a handle with a scenario bank: what imgenv_world_scenarios answers for the worlds of this reset
static int reset_scenario_mark(imgenv* h, const int* list, int n, const ResetChoices& choices, hipStream_t st) {
    const int n_mark = list ? n : h->W;
    int* ids = nullptr;
    if (choices.scn_ids) RTRY(stage_ints(h, choices.scn_ids, (size_t)n_mark, &ids));
    k_scenario_mark<<<dim3((unsigned)((n_mark + 255) / 256)), dim3(256), 0, st>>>(h->d_scn_world, h->d_scn_mark, h->dev.ready ? h->dev.pool.place_serial : nullptr,
                                                                                  list ? h->rs.list : nullptr, ids, n_mark);
    return 0;
}
// The one bracket of a reset chain: while `body` runs, the handle's launches cover the listed worlds (a device pointer; n_dev: the
// list's length lives on the device and n is its capacity), afterwards every world again -- however body ends.
template <typename Body>
static int with_active(imgenv* h, const int* list, int n, const int* n_dev, Body&& body) {
    set_active(h, list, n);
    h->d.act_n_dev = n_dev;
    const int rc = body();
    set_active(h, nullptr, 0);
    h->d.act_n_dev = nullptr;
    return rc;
}

static int sfm_ahead_drop(imgenv* h, hipStream_t st);
// commit, 5: the launches
static int reset_launch(imgenv* h, const int* list, int n, bool whole_wobst, const ResetChoices& choices, hipStream_t st, int whole) {
    if (int rc = sfm_ahead_drop(h, st)) return rc;  // (a reset writes the live crowd: positions, waypoints)
    RTRY(reset_stage_tables(h, list, n, whole_wobst));
    size_t n_inst = 0;
    RTRY(reset_stage_obstacles(h, list ? n : h->W, &n_inst));
    const int rc = with_active(h, list ? h->d_act_list : nullptr, n, nullptr, [&]() -> int {
        const DevWorld& d = h->d;
        const ResetPlan rp = plan_reset(h->plan, chain_facts(h, 1), h->rs.segs.size(), h->rs.seg_max, n_inst);
        RTRY(reset_apply(h, rp, choices, st, whole));
        if (n_inst)
            k_reset_obstacles_for(h->plan)<<<dim3(rp.obstacles.grid), dim3(rp.obstacles.block), 0, st>>>(d, h->rs.d_inst, h->plan.layer, nullptr, 0, 1, nullptr, nullptr);
        if (d.sharded) k_reset_bbox<<<dim3(rp.bbox.grid), dim3(rp.bbox.block), 0, st>>>(d, h->rs.rob3);
        const bool fed = !h->rs.fed.empty();
        if (fed) RTRY(reset_tracks(h, st));
        if (h->d_scn_world) RTRY(reset_scenario_mark(h, list, n, choices, st));
        HIPCHK(hipGetLastError());
        h->launches = 2 + (fed ? 1 : 0) + (h->d_scn_world ? 1 : 0);
        return launch_views(h, st, 1);
    });
    // k_reset_apply is in flight and reads this generation's page-locked chunks: mark them pending whatever came after
    const int rc_end = stage_end(h, st);
    return rc ? rc : rc_end;
}
// commit: the n prepared worlds (list == nullptr: every world, world k from its share of the one batch)
static int reset_commit(imgenv* h, const ResetFacts& f, int n, const int32_t* list, const imgenv_reset_batch* batches, const ResetChoices& choices,
                        hipStream_t st, double* stage_us) {
    const auto t0 = std::chrono::steady_clock::now();
    const ResetGrowth g = reset_growth(f, h->rs.worlds.data(), n);
    RTRY(reset_grow(h, g, st));
    RTRY(stage_rvo(h, list, n, g));
    for (int q = 0; q < n; q++) {
        const imgenv_reset_batch sub = list ? batches[q] : world_batch(h, batches, q);
        RTRY(stage_world(h, f, h->rs.worlds[q], q, &sub, choices, list ? h->elapsed : 0));
    }
    if (!list) {
        if (h->d.sharded) {
            const uint32_t init[4] = {BBOX_INIT_MIN, BBOX_INIT_MIN, BBOX_INIT_MAX, BBOX_INIT_MAX};
            RTRY(stage_put(h, h->d.bbox, init, sizeof(init)));
        }
        h->elapsed = 0;  // TimeLimitWrapper.reset (base.py:229-231)
        h->dev.used = false;  // every world's host copy is current again
    }
    if (stage_us) *stage_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    return reset_launch(h, list, list ? n : 0, g.rvo_moved, choices, st, list ? 0 : 1);  // no host wait: the copies read the handle's pinned chunks
}

// every world of the handle from one batch; `choices` hold one entry per world (a handle of one world: what its host-placed reset drew)
static int reset_all(imgenv* h, const imgenv_reset_batch* b, const ResetChoices& choices, hipStream_t st) {
    if (!h) FAIL(IMGENV_EINVAL, "null argument");
    const ResetFacts f = reset_facts(h);
    RTRY(reset_check_batches(f, 1, b, h->P, g_err));
    RTRY(reset_prepare(h, f, h->W, nullptr, b));
    RTRY(reset_device_ready(h, st));
    RTRY(stage_begin(h));
    RTRY(reset_blocks(h, h->W, nullptr));
    RTRY(reset_commit(h, f, h->W, nullptr, b, choices, st, nullptr));
    h->has_reset = true;
    return IMGENV_OK;
}

extern "C" int imgenv_reset(imgenv_t* h, const imgenv_reset_batch* b, void* stream) { return reset_all(h, b, ResetChoices(), (hipStream_t)stream); }

// the listed worlds, each from its batch; `choices` in list order
static int reset_worlds(imgenv* h, int n, const int32_t* worlds, const imgenv_reset_batch* batches, const ResetChoices& choices, hipStream_t st) {
    if (n <= 0) return h ? IMGENV_OK : IMGENV_EINVAL;
    if (!h || !worlds) FAIL(IMGENV_EINVAL, "null argument");
    const ResetFacts f = reset_facts(h);
    RTRY(reset_check_batches(f, n, batches, h->Pw, g_err));
    if (!world_list_check(h->W, n, worlds, nullptr, 0, nullptr, &g_err)) return IMGENV_EINVAL;
    if (h->W == 1) return reset_all(h, batches, choices, st);  // (the list is {0}: one entry of every choice)
    const bool trace = imgenv::ResetTrace::on();
    double us[3] = {0, 0, 0}, t[3] = {0, 0, 0};  // begin, stage worlds (prepare included), launches
    if (trace) t[0] = imgenv::ResetTrace::now_us();
    RTRY(reset_prepare(h, f, n, worlds, batches));
    if (trace) t[1] = imgenv::ResetTrace::now_us();
    RTRY(reset_device_ready(h, st));
    RTRY(stage_begin(h));
    RTRY(reset_blocks(h, n, worlds));
    if (trace) t[2] = imgenv::ResetTrace::now_us();
    RTRY(reset_commit(h, f, n, worlds, batches, choices, st, &us[1]));
    if (trace) {
        us[0] = t[2] - t[1];
        us[2] = imgenv::ResetTrace::now_us() - t[2] - us[1];
        us[1] += t[1] - t[0];
        imgenv::ResetTrace& tr = h->rs.trace;
        if (tr.add(us, 3, n))
            fprintf(stderr, "[imgenv_reset_worlds] %ld calls, %.1f worlds/call: begin %.1f us, stage worlds %.1f us, launches %.1f us per call\n",
                    tr.calls, (double)tr.worlds / tr.calls, tr.acc[0] / tr.calls, tr.acc[1] / tr.calls, tr.acc[2] / tr.calls);
    }
    bool all = true;
    for (char r : h->world_ready) all = all && r;
    h->has_reset = all;
    return IMGENV_OK;
}

extern "C" int imgenv_reset_worlds(imgenv_t* h, int32_t n, const int32_t* worlds, const imgenv_reset_batch* batches, void* stream) {
    return reset_worlds(h, n, worlds, batches, ResetChoices(), (hipStream_t)stream);
}

// the draws of n host-placed resets from their seeds (null: seed0 + q) under the handle's BY_PLACEMENT policies
static PlacementDraws placement_draws(const imgenv* h, int n, const uint64_t* seeds, uint64_t seed0) {
    return PlacementDraws(n, seeds, seed0, h->d_map_cur && h->maps_policy == IMGENV_MAPS_BY_PLACEMENT ? h->n_maps : 0,
                          h->d_trk_cur && h->tracks_policy == IMGENV_TRACKS_BY_PLACEMENT ? h->n_track_sets : 0);
}

static int spawn_cfg_check(const imgenv_spawn_cfg* c) {
    if (!c) FAIL(IMGENV_EINVAL, "null argument");
    if (c->struct_size != (int32_t)sizeof(imgenv_spawn_cfg)) FAIL(IMGENV_EINVAL, "spawn cfg ABI mismatch");
    if (c->n_robots < 0 || c->n_peds < 0 || c->n_obstacles < 0 || (c->n_robots + c->n_peds > 0 && !c->agents) ||
        (c->n_obstacles > 0 && !c->obstacles) || !(c->clearance >= 0))
        FAIL(IMGENV_EINVAL, "bad spawn cfg");
    for (int i = 0; i < c->n_robots + c->n_peds; i++) {
        const imgenv_spawn_agent& a = c->agents[i];
        const bool begin_ok = (a.begin_type >= IMGENV_POSE_FIX && a.begin_type <= IMGENV_POSE_RANGE_YAW) ||
                              a.begin_type == IMGENV_POSE_RANGE_CIRCLE || a.begin_type == IMGENV_POSE_RANGE_CIRCLE_FIX ||
                              a.begin_type == IMGENV_POSE_RANGE_MULTI;
        const bool target_ok = a.target_type >= IMGENV_POSE_FIX && a.target_type <= IMGENV_POSE_RANGE_MULTI;
        if (!begin_ok || !target_ok)
            FAIL(IMGENV_EINVAL, "agent %d: unsupported pose type (%d, %d)", i, a.begin_type, a.target_type);
    }
    return 0;
}

extern "C" int imgenv_spawn(const imgenv_spawn_cfg* cfg, uint64_t seed, double* robot_pose, double* robot_goal, double* ped_pose,
                            double* ped_goal, double* ped_traj, int32_t* ped_traj_len, int32_t* obs_shape, float* obs_size,
                            double* obs_pose) {
    if (int rc = spawn_cfg_check(cfg)) return rc;
    SpawnOut o;
    if (const char* why = spawn_world(*cfg, seed, o)) FAIL(IMGENV_EINVAL, "spawn: %s", why);
    const size_t R = cfg->n_robots, P = cfg->n_peds, O = cfg->n_obstacles;
    if (robot_pose) memcpy(robot_pose, o.robot_pose.data(), sizeof(double) * 4 * R);
    if (robot_goal) memcpy(robot_goal, o.robot_goal.data(), sizeof(double) * 2 * R);
    if (ped_pose) memcpy(ped_pose, o.ped_pose.data(), sizeof(double) * 4 * P);
    if (ped_goal) memcpy(ped_goal, o.ped_goal.data(), sizeof(double) * 2 * P);
    if (ped_traj) memcpy(ped_traj, o.ped_traj.data(), sizeof(double) * 6 * P);
    if (ped_traj_len) memcpy(ped_traj_len, o.ped_traj_len.data(), sizeof(int32_t) * P);
    if (obs_shape) memcpy(obs_shape, o.obs_shape.data(), sizeof(int32_t) * O);
    if (obs_size) memcpy(obs_size, o.obs_size.data(), sizeof(float) * 4 * O);
    if (obs_pose) memcpy(obs_pose, o.obs_pose.data(), sizeof(double) * 4 * O);
    return IMGENV_OK;
}

extern "C" int imgenv_reset_worlds_spawn(imgenv_t* h, int32_t n, const int32_t* worlds, const imgenv_spawn_cfg* cfg,
                                         const uint64_t* seeds, void* stream) {
    if (!h || !worlds || !seeds) FAIL(IMGENV_EINVAL, "null argument");
    if (int rc = spawn_cfg_check(cfg)) return rc;
    if (cfg->n_robots != h->Rw || cfg->n_peds != h->Pw)
        FAIL(IMGENV_EINVAL, "spawn cfg is for %d robots / %d pedestrians, a world of this handle has %d / %d", cfg->n_robots,
             cfg->n_peds, h->Rw, h->Pw);
    if (n <= 0) return IMGENV_OK;
    std::vector<SpawnOut> outs((size_t)n);
    std::vector<imgenv_reset_batch> batches((size_t)n);
    for (int q = 0; q < n; q++) {
        if (const char* why = spawn_world(*cfg, seeds[q], outs[q])) FAIL(IMGENV_EINVAL, "spawn of world %d: %s", worlds[q], why);
        batches[q] = outs[q].batch;
    }
    const PlacementDraws draws = placement_draws(h, n, seeds, 0);  // the placement's seed also draws the map and the recorded crowd
    return reset_worlds(h, n, worlds, batches.data(), draws.choices(), (hipStream_t)stream);
}

extern "C" int imgenv_reset_world(imgenv_t* h, int32_t world, const imgenv_reset_batch* b, void* stream) {
    return imgenv_reset_worlds(h, 1, &world, b, stream);
}

// ---------------------------------------------------------------------------------------- map bank
extern "C" int32_t imgenv_map_for_placement(uint64_t seed, int32_t n_maps) { return map_for_placement(seed, n_maps); }

extern "C" int imgenv_maps_add(imgenv_t* h, int32_t n, const uint8_t* maps, int32_t Hg, int32_t Wg) {
    if (!h || !maps || n < 1) FAIL(IMGENV_EINVAL, "null argument or no maps");
    if (h->n_maps > 1) FAIL(IMGENV_ESTATE, "imgenv_maps_add has already been called on this handle");
    if (any_world_reset(h)) FAIL(IMGENV_ESTATE, "imgenv_maps_add after the first reset");
    if (h->RL != h->R) FAIL(IMGENV_EINVAL, "imgenv_maps_add on a robot shard is not supported");
    if (Hg != h->Hg_in || Wg != h->Wg_in)
        FAIL(IMGENV_EINVAL, "maps of %d x %d pixels, the handle was created with %d x %d: one size per handle", Hg, Wg, h->Hg_in, h->Wg_in);
    if (n > (1 << 20)) FAIL(IMGENV_EINVAL, "too many maps");
    HIPCHK(hipSetDevice(h->cfg.device));
    const int n_maps = n + 1, W = h->W;
    const size_t G = (size_t)h->Hg * h->Wg, G_in = (size_t)Hg * Wg, stride = h->map_stride;
    const bool resize = h->Hg != Hg || h->Wg != Wg || h->cfg.global_resolution != h->cfg.view_resolution;
    DevWorld& d = h->d;
    // everything is allocated and filled before the handle changes: a failure leaves it on its one map
    DevTxn<HipApi> txn;
    uint8_t* bank = nullptr;
    uint8_t* crops = nullptr;
    int *cur = nullptr, *next = nullptr;
    txn.room(&bank, stride * (size_t)n_maps, 0);
    txn.copy(bank, h->d_static_map, stride);  // map 0: the map of imgenv_create
    if (d.crop_map) {
        txn.room(&crops, (size_t)d.crop_ws * n_maps, 0);
        txn.copy(crops, d.static_crop, (size_t)d.crop_ws);
    }
    std::vector<uint8_t> resized, tiled;
    for (int k = 0; k < n && txn.code() == IMGENV_OK; k++) {
        const uint8_t* src = maps + (size_t)k * G_in;
        if (resize) {  // GridMap::read_image (grid_map.cpp:28-38), as imgenv_create does for the first map
            resized.resize(G);
            cv_resize_u8(false, src, Hg, Wg, resized.data(), h->Hg, h->Wg);
            src = resized.data();
        }
        txn.put(bank + (size_t)(k + 1) * stride, src, G);
        if (crops) {
            tile_crop(src, h->Hg, h->Wg, d.crop_wt, (size_t)d.crop_ws, tiled);
            txn.put(crops + (size_t)(k + 1) * d.crop_ws, tiled.data(), tiled.size());
        }
    }
    txn.room(&cur, (size_t)W, 0);  // (zeroed: every world starts on map 0)
    txn.room(&next, (size_t)W, 0);
    if (txn.code()) FAIL(txn.code(), "imgenv_maps_add: a bank of %d maps: %s", n_maps, txn.error());
    txn.commit(h->allocs);
    // (nothing has been launched on this handle yet -- no reset has happened -- so the single-map buffers can go)
    dev_free(h, h->d_static_map);
    h->d_static_map = bank;
    if (crops) {
        uint8_t* old = const_cast<uint8_t*>(d.static_crop);
        dev_free(h, old);
        d.static_crop = crops;
    }
    h->d_map_cur = cur;
    h->d_map_next = next;
    h->n_maps = n_maps;
    return IMGENV_OK;
}

// imgenv_world_maps_set / imgenv_world_tracks_set behind their checks: next[worlds[q]] = ids[q] for the n > 0 listed worlds, by one
// small launch on the caller's stream that reads the lists from page-locked memory
static int world_select(imgenv* h, int* next, int n, const int32_t* worlds, const int32_t* ids, hipStream_t st) {
    HIPCHK(hipSetDevice(h->cfg.device));
    RTRY(stage_begin(h));
    unsigned char* p = nullptr;
    RTRY(stage_room(h, sizeof(int) * 2 * (size_t)n, &p));
    int* pin = (int*)p;
    memcpy(pin, worlds, sizeof(int) * (size_t)n);
    memcpy(pin + n, ids, sizeof(int) * (size_t)n);
    k_world_select<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st>>>(next, pin, pin + n, n);
    HIPCHK(hipGetLastError());
    return stage_end(h, st);
}

// imgenv_world_maps / imgenv_world_tracks: the [W] array `cur` once the stream has drained; a handle without that bank answers `fallback`
static int world_ids_read(imgenv* h, const int* cur, int fallback, int32_t* out, hipStream_t st) {
    if (!h || !out) FAIL(IMGENV_EINVAL, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipStreamSynchronize(st));
    if (int rc = check_device_flags(h)) return rc;
    if (!cur) std::fill_n(out, h->W, fallback);
    else HIPCHK(hipMemcpy(out, cur, sizeof(int) * (size_t)h->W, hipMemcpyDeviceToHost));
    return IMGENV_OK;
}

extern "C" int imgenv_world_maps_set(imgenv_t* h, int32_t n, const int32_t* worlds, const int32_t* map_ids, void* stream) {
    if (!h || n < 0 || (n > 0 && (!worlds || !map_ids))) FAIL(IMGENV_EINVAL, "null argument");
    if (!world_list_check(h->W, n, worlds, map_ids, h->n_maps, "map", &g_err)) return IMGENV_EINVAL;  // (before anything is applied)
    if (n == 0 || !h->d_map_next) return IMGENV_OK;  // (one map: every id is 0)
    return world_select(h, h->d_map_next, n, worlds, map_ids, (hipStream_t)stream);
}

extern "C" int imgenv_maps_policy(imgenv_t* h, int32_t policy) {
    if (!h) FAIL(IMGENV_EINVAL, "null argument");
    if (policy != IMGENV_MAPS_KEEP && policy != IMGENV_MAPS_BY_PLACEMENT) FAIL(IMGENV_EINVAL, "unknown map policy %d", policy);
    h->maps_policy = policy;
    return IMGENV_OK;
}

extern "C" int imgenv_world_maps(imgenv_t* h, int32_t* map_ids, void* stream) {
    return world_ids_read(h, h ? h->d_map_cur : nullptr, 0, map_ids, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------- track bank
extern "C" int32_t imgenv_tracks_for_placement(uint64_t seed, int32_t n_sets) { return tracks_for_placement(seed, n_sets); }

extern "C" int imgenv_tracks_add(imgenv_t* h, int32_t n_sets, int32_t cap, const double* ped_pose, const double* ped_traj,
                                 const double* ped_traj_v, const int32_t* ped_traj_len) {
    if (!h || !ped_pose || !ped_traj || !ped_traj_v || !ped_traj_len) FAIL(IMGENV_EINVAL, "null argument");
    if (h->n_track_sets > 0) FAIL(IMGENV_ESTATE, "imgenv_tracks_add has already been called on this handle");
    if (any_world_reset(h)) FAIL(IMGENV_ESTATE, "imgenv_tracks_add after the first reset");
    if (h->cfg.ped_scene_type != IMGENV_SCENE_DATASET) FAIL(IMGENV_EINVAL, "imgenv_tracks_add: the pedestrian scene is not IMGENV_SCENE_DATASET");
    if (h->Pw < 1) FAIL(IMGENV_EINVAL, "imgenv_tracks_add: the handle has no pedestrians");
    if (h->RL != h->R) FAIL(IMGENV_EINVAL, "imgenv_tracks_add on a robot shard is not supported");
    if (n_sets < 1 || n_sets > (1 << 20) || cap < 1 || cap > (1 << 24)) FAIL(IMGENV_EINVAL, "imgenv_tracks_add: %d sets of %d records", n_sets, cap);
    const int Pw = h->Pw, stride = std::max(cap, 2);
    const size_t words = (size_t)Pw * stride * 3;
    // every set as a reset would stage it (track_bank.h), on the host first: a bad set fails the call before anything is allocated
    std::vector<double> pose3((size_t)n_sets * Pw * 3), traj((size_t)n_sets * words), traj_v((size_t)n_sets * words);
    std::vector<int32_t> len((size_t)n_sets * Pw);
    for (int s = 0; s < n_sets; s++) {
        const int bad = tracks_convert_set(Pw, cap, stride, ped_pose + (size_t)s * Pw * 4, ped_traj + (size_t)s * Pw * cap * 3,
                                           ped_traj_v + (size_t)s * Pw * cap * 2, ped_traj_len + (size_t)s * Pw, pose3.data() + (size_t)s * Pw * 3,
                                           traj.data() + (size_t)s * words, traj_v.data() + (size_t)s * words, len.data() + (size_t)s * Pw);
        if (bad > 0) FAIL(IMGENV_EINVAL, "imgenv_tracks_add: set %d, pedestrian %d: bad trajectory length %d (cap %d)", s, bad - 1, ped_traj_len[(size_t)s * Pw + bad - 1], cap);
        if (bad < 0) FAIL(IMGENV_EINVAL, "imgenv_tracks_add: set %d, pedestrian %d: a value that is not finite", s, -bad - 1);
    }
    HIPCHK(hipSetDevice(h->cfg.device));
    // everything is allocated and filled before the handle changes: a failure leaves it without a bank
    double *b_traj = nullptr, *b_traj_v = nullptr, *b_pose3 = nullptr, *t_traj = nullptr, *t_traj_v = nullptr;
    int *b_len = nullptr, *cur = nullptr, *next = nullptr;
    uint32_t* count = nullptr;
    DevTxn<HipApi> txn;
    const size_t P = (size_t)h->P, W = (size_t)h->W;
    txn.room(&b_traj, traj.size(), 0);
    txn.room(&b_traj_v, traj_v.size(), 0);
    txn.room(&b_pose3, pose3.size(), 0);
    txn.room(&b_len, len.size(), 0);
    txn.room(&cur, W, 0xFF);
    txn.room(&next, W, 0);
    txn.room(&count, W, 0);
    if (h->traj_cap < stride) {
        txn.room(&t_traj, P * stride * 3, 0);
        txn.room(&t_traj_v, P * stride * 3, 0);
    }
    txn.put(b_traj, traj.data(), 8 * traj.size());
    txn.put(b_traj_v, traj_v.data(), 8 * traj_v.size());
    txn.put(b_pose3, pose3.data(), 8 * pose3.size());
    txn.put(b_len, len.data(), 4 * len.size());
    if (txn.code()) FAIL(txn.code(), "imgenv_tracks_add: a bank of %d track sets: %s", n_sets, txn.error());
    txn.commit(h->allocs);
    if (t_traj) {  // the per-world tables with room for a set, so that the first reset finds them (no reset has happened: nothing reads the old ones)
        dev_free(h, h->d_traj);
        dev_free(h, h->d_traj_v);
        h->d_traj = t_traj;
        h->d_traj_v = t_traj_v;
        h->traj_cap = stride;
    }
    h->d.ptraj = h->d_traj;
    h->d.ptraj_v = h->d_traj_v;
    h->d.traj_cap = h->traj_cap;
    h->d_trk_traj = b_traj; h->d_trk_traj_v = b_traj_v; h->d_trk_pose3 = b_pose3; h->d_trk_len = b_len;
    h->d_trk_cur = cur; h->d_trk_next = next; h->d_trk_count = count;
    h->n_track_sets = n_sets;
    h->trk_cap = stride;
    return IMGENV_OK;
}

extern "C" int imgenv_world_tracks_set(imgenv_t* h, int32_t n, const int32_t* worlds, const int32_t* set_ids, void* stream) {
    if (!h || n < 0 || (n > 0 && (!worlds || !set_ids))) FAIL(IMGENV_EINVAL, "null argument");
    if (!h->d_trk_next) FAIL(IMGENV_ESTATE, "imgenv_world_tracks_set: the handle has no track bank (imgenv_tracks_add)");
    if (!world_list_check(h->W, n, worlds, set_ids, h->n_track_sets, "track set", &g_err)) return IMGENV_EINVAL;  // (before anything is applied)
    if (n == 0) return IMGENV_OK;
    return world_select(h, h->d_trk_next, n, worlds, set_ids, (hipStream_t)stream);
}

extern "C" int imgenv_tracks_policy(imgenv_t* h, int32_t policy, int32_t repeat) {
    if (!h) FAIL(IMGENV_EINVAL, "null argument");
    if (policy != IMGENV_TRACKS_KEEP && policy != IMGENV_TRACKS_BY_PLACEMENT && policy != IMGENV_TRACKS_CYCLE) FAIL(IMGENV_EINVAL, "unknown track policy %d", policy);
    if (repeat < 1) FAIL(IMGENV_EINVAL, "imgenv_tracks_policy: repeat %d (at least 1)", repeat);
    if (!h->d_trk_count) FAIL(IMGENV_ESTATE, "imgenv_tracks_policy: the handle has no track bank (imgenv_tracks_add)");
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipDeviceSynchronize());  // (resets in flight still count with the old policy)
    HIPCHK(hipMemset(h->d_trk_count, 0, sizeof(uint32_t) * (size_t)h->W));
    HIPCHK(hipDeviceSynchronize());
    h->tracks_policy = policy;
    h->tracks_repeat = repeat;
    return IMGENV_OK;
}

extern "C" int imgenv_world_tracks(imgenv_t* h, int32_t* set_ids, void* stream) {
    return world_ids_read(h, h ? h->d_trk_cur : nullptr, -1, set_ids, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------- scenario bank
extern "C" int32_t imgenv_scenario_for_placement(int32_t policy, uint64_t seed0, uint64_t first, uint64_t n, int32_t n_scenarios) {
    return scenario_for_placement(policy, seed0, first, n, n_scenarios);
}

extern "C" int imgenv_scenarios_add(imgenv_t* h, int32_t n, int32_t n_obstacles, const double* robot_pose, const double* robot_goal,
                                    const double* ped_pose, const double* ped_goal, const double* ped_traj, const int32_t* ped_traj_len,
                                    const int32_t* obs_shape, const float* obs_size, const double* obs_pose) {
    if (!h || !robot_pose || !robot_goal) FAIL(IMGENV_EINVAL, "null argument");
    if (h->n_scn > 0) FAIL(IMGENV_ESTATE, "imgenv_scenarios_add has already been called on this handle");
    if (h->dev.ready) FAIL(IMGENV_ESTATE, "imgenv_scenarios_add after the first imgenv_step_autoreset_device");
    if (h->RL != h->R) FAIL(IMGENV_EINVAL, "imgenv_scenarios_add on a robot shard is not supported");
    const int Rw = h->Rw, Pw = h->Pw, na = Rw + Pw, O = n_obstacles;
    if (n < 1 || n > (1 << 24)) FAIL(IMGENV_EINVAL, "imgenv_scenarios_add: %d scenarios", n);
    if (O < 0 || O > SPAWN_MAX_OBST || na > SPAWN_MAX_AGENTS)
        FAIL(IMGENV_EINVAL, "imgenv_scenarios_add: %d agents and %d obstacles per world, the device-side reset places at most %d and %d", na, O,
             SPAWN_MAX_AGENTS, SPAWN_MAX_OBST);
    if (Pw > 0 && (!ped_pose || !ped_goal || !ped_traj || !ped_traj_len)) FAIL(IMGENV_EINVAL, "imgenv_scenarios_add: null pedestrian arrays");
    if (O > 0 && (!obs_shape || !obs_size || !obs_pose)) FAIL(IMGENV_EINVAL, "imgenv_scenarios_add: null obstacle arrays");
    // the whole bank on the host first: bad input fails the call before anything is allocated
    std::vector<SlotAgent> agents((size_t)n * std::max(na, 1));
    std::vector<SlotObstacle> obst((size_t)n * std::max(O, 1));
    int where = 0, which = 0;
    if (const int bad = scenarios_convert(n, Rw, Pw, O, robot_pose, robot_goal, ped_pose, ped_goal, ped_traj, ped_traj_len, obs_shape, obs_size,
                                          obs_pose, agents.data(), obst.data(), &where, &which))
        FAIL(IMGENV_EINVAL, "imgenv_scenarios_add: scenario %d, %s %d: %s", where,
             bad >= SCENARIO_BAD_SHAPE ? "obstacle" : (which < Rw ? "robot" : "pedestrian"), bad >= SCENARIO_BAD_SHAPE || which < Rw ? which : which - Rw,
             scenario_error_text(bad));
    if (na > 0) agents.resize((size_t)n * na);
    if (O > 0) obst.resize((size_t)n * O);
    if (h->NA > 0 && O > 0) {  // RVO agents: every scenario's polygons and their BSP, built by the device BSP's host twin, must fit a slot
        const int cap = spawn_slot_cap(O);
        RvoObstacles rvo;
        for (int s = 0; s < n; s++) {
            rvo.clear();
            for (int q = 0; q < O; q++) {
                const SlotObstacle& o = obst[(size_t)s * O + q];
                const double sizes[4] = {(double)o.size[0], (double)o.size[1], (double)o.size[2], (double)o.size[3]};
                const double yaw = tf_yaw_from_quaternion_zw(o.qz, o.qw);
                double seg[4];
                float v[8];
                obstacle_polygon(o.shape, sizes, o.x, o.y, sin(yaw * 0.5), cos(yaw * 0.5), seg, v);
                rvo.add(v, 4);
            }
            rvo.process();
            if ((int)rvo.ob.size() > cap || (int)rvo.nodes.size() > cap)
                FAIL(IMGENV_EINVAL, "imgenv_scenarios_add: scenario %d: %d RVO obstacle vertices and %d BSP nodes, a pool slot has room for %d", s,
                     (int)rvo.ob.size(), (int)rvo.nodes.size(), cap);
        }
    }
    HIPCHK(hipSetDevice(h->cfg.device));
    SlotAgent* da = nullptr;
    SlotObstacle* dob = nullptr;
    int* scn = nullptr;
    unsigned long long *mark = nullptr, *starts = nullptr;
    const size_t starts_cap = 256;
    DevTxn<HipApi> txn;  // everything is allocated and filled before the handle changes: a failure leaves it without a bank
    txn.room(&da, agents.size(), 0);
    txn.room(&dob, obst.size(), 0);
    txn.room(&scn, (size_t)h->W, 0xFF);
    txn.room(&mark, (size_t)h->W, 0xFF);
    txn.room(&starts, starts_cap, 0);
    txn.put(da, agents.data(), sizeof(SlotAgent) * agents.size());
    txn.put(dob, obst.data(), sizeof(SlotObstacle) * obst.size());
    if (txn.code()) FAIL(txn.code(), "imgenv_scenarios_add: a bank of %d scenarios: %s", n, txn.error());
    txn.commit(h->allocs);
    h->scn_agents.swap(agents);
    h->scn_obstacles.swap(obst);
    h->d_scn_agents = da; h->d_scn_obst = dob; h->d_scn_world = scn; h->d_scn_mark = mark;
    h->d_scn_starts = starts; h->scn_starts_cap = starts_cap;
    h->n_scn = n;
    h->scn_obst = O;
    h->scn_policy = IMGENV_SCENARIOS_OFF;
    h->scn_first = 0;
    h->scn_epochs.assign(1, imgenv::ScnEpoch{IMGENV_SCENARIOS_OFF, 0});  // (epoch 0 starts at placement 0: the array is zeroed)
    return IMGENV_OK;
}

extern "C" int imgenv_scenarios_policy(imgenv_t* h, int32_t policy, uint64_t first, void* stream) {
    if (!h) FAIL(IMGENV_EINVAL, "null argument");
    if (policy != IMGENV_SCENARIOS_OFF && policy != IMGENV_SCENARIOS_QUEUE && policy != IMGENV_SCENARIOS_BY_PLACEMENT)
        FAIL(IMGENV_EINVAL, "unknown scenario policy %d", policy);
    if (h->n_scn < 1) FAIL(IMGENV_ESTATE, "imgenv_scenarios_policy: the handle has no scenario bank (imgenv_scenarios_add)");
    hipStream_t st = (hipStream_t)stream;
    if (h->dev.ready) {
        // The pool's slots were drawn under the old policy and must not be handed out: every slot loses its serial on the caller's
        // stream and the next chain's fill -- forced, behind this on the chain's event -- draws them again (spawn_dev_refresh's
        // stride path does the same).  The placements from the device's present count on belong to the new policy: the count is
        // copied on the device, for imgenv_world_scenarios.  Nothing here waits for the device.
        HIPCHK(hipSetDevice(h->cfg.device));
        SpawnDev& c = h->dev.pool;
        if (h->scn_epochs.size() >= h->scn_starts_cap) {  // (every 256th switch and rarer: the log doubles; the old block lives until imgenv_destroy)
            unsigned long long* grown = nullptr;
            RTRY(dev_alloc(h, &grown, h->scn_starts_cap * 2));
            HIPCHK(hipMemcpyAsync(grown, h->d_scn_starts, sizeof(unsigned long long) * h->scn_starts_cap, hipMemcpyDeviceToDevice, st));
            h->d_scn_starts = grown;
            h->scn_starts_cap *= 2;
        }
        HIPCHK(hipMemcpyAsync(h->d_scn_starts + h->scn_epochs.size(), c.consumed, sizeof(unsigned long long), hipMemcpyDeviceToDevice, st));
        h->scn_epochs.push_back(imgenv::ScnEpoch{policy, first});
        HIPCHK(hipMemsetAsync(c.slot_serial, 0xFF, sizeof(unsigned long long) * (size_t)c.S, st));
        h->dev.fill_due = 0;
    } else {  // no pool yet: its first fill takes the policy, from placement 0
        h->scn_epochs.assign(1, imgenv::ScnEpoch{policy, first});
    }
    h->scn_policy = policy;
    h->scn_first = first;
    return IMGENV_OK;
}

extern "C" int imgenv_reset_worlds_scenarios(imgenv_t* h, int32_t n, const int32_t* worlds, const int32_t* ids, void* stream) {
    if (!h || n < 0 || (n > 0 && (!worlds || !ids))) FAIL(IMGENV_EINVAL, "null argument");
    if (h->n_scn < 1) FAIL(IMGENV_ESTATE, "imgenv_reset_worlds_scenarios: the handle has no scenario bank (imgenv_scenarios_add)");
    if (!world_list_check(h->W, n, worlds, ids, h->n_scn, "scenario", &g_err)) return IMGENV_EINVAL;  // (the ids index the bank's host copy below)
    if (n == 0) return IMGENV_OK;
    const int Rw = h->Rw, Pw = h->Pw, O = h->scn_obst, na = Rw + Pw;
    // the batches of imgenv_reset_worlds, out of the bank's host copy (trajectories of two points, as imgenv_spawn lays them out)
    const size_t N = (size_t)n;
    std::vector<double> rp(N * Rw * 4 + 1), rg(N * Rw * 2 + 1), pp(N * Pw * 4 + 1), pg(N * Pw * 2 + 1), pt(N * Pw * 6 + 1), op(N * O * 4 + 1);
    std::vector<int32_t> pl(N * Pw + 1), os(N * O + 1);
    std::vector<float> oz(N * O * 4 + 1);
    std::vector<imgenv_reset_batch> batches(N);
    for (size_t q = 0; q < N; q++) {
        const size_t id = (size_t)ids[q];
        scenario_to_arrays(Rw, Pw, O, h->scn_agents.data() + id * na, h->scn_obstacles.data() + id * O, rp.data() + q * Rw * 4, rg.data() + q * Rw * 2,
                           pp.data() + q * Pw * 4, pg.data() + q * Pw * 2, pt.data() + q * Pw * 6, pl.data() + q * Pw, os.data() + q * O,
                           oz.data() + q * O * 4, op.data() + q * O * 4);
        imgenv_reset_batch& b = batches[q];
        memset(&b, 0, sizeof(b));
        b.struct_size = (int32_t)sizeof(b);
        b.n_obstacles = O;
        b.obs_shape = os.data() + q * O; b.obs_size = oz.data() + q * O * 4; b.obs_pose = op.data() + q * O * 4;
        b.robot_pose = rp.data() + q * Rw * 4; b.robot_goal = rg.data() + q * Rw * 2;
        b.ped_pose = pp.data() + q * Pw * 4; b.ped_goal = pg.data() + q * Pw * 2;
        b.ped_traj_len = pl.data() + q * Pw; b.ped_traj = pt.data() + q * Pw * 6;
        b.ped_traj_cap = 2;
    }
    return reset_worlds(h, n, worlds, batches.data(), ResetChoices{nullptr, nullptr, ids}, (hipStream_t)stream);
}

// Which scenario the device handed out for a placement number (imgenv_world_scenarios, imgenv_episode_log_read): the starts of the
// policy's epochs, as the device counted them, pulled once per call ...
static int scenario_starts_pull(const imgenv* h, std::vector<unsigned long long>& starts) {
    starts.resize(h->scn_epochs.size());
    HIPCHK(hipMemcpy(starts.data(), h->d_scn_starts, sizeof(unsigned long long) * starts.size(), hipMemcpyDeviceToHost));
    return IMGENV_OK;
}
// ... and the placement under the policy of the epoch it falls into
static int32_t scenario_of_placement(const imgenv* h, const std::vector<unsigned long long>& starts, uint64_t serial) {
    const imgenv::ScnEpoch& e = h->scn_epochs[scenario_epoch_of(starts.data(), starts.size(), serial)];
    const uint64_t seed0 = h->dev.ready ? h->dev.pool.seed0 : 0;
    return scenario_for_placement(e.policy, seed0, e.first, serial, h->n_scn);
}

extern "C" int imgenv_world_scenarios(imgenv_t* h, int32_t* ids, void* stream) {
    if (!h || !ids) FAIL(IMGENV_EINVAL, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    if (int rc = check_device_flags(h)) return rc;
    const size_t W = (size_t)h->W;
    for (size_t k = 0; k < W; k++) ids[k] = -1;
    if (h->n_scn < 1) return IMGENV_OK;
    std::vector<int> scn(W);
    std::vector<unsigned long long> mark(W), serial(W, ~0ull), starts;
    HIPCHK(hipMemcpy(scn.data(), h->d_scn_world, sizeof(int) * W, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(mark.data(), h->d_scn_mark, sizeof(unsigned long long) * W, hipMemcpyDeviceToHost));
    RTRY(scenario_starts_pull(h, starts));
    if (h->dev.ready)
        HIPCHK(hipMemcpy(serial.data(), h->dev.pool.place_serial, sizeof(unsigned long long) * W, hipMemcpyDeviceToHost));
    for (size_t k = 0; k < W; k++)  // (equal: the host reset it last, or nobody has)
        ids[k] = serial[k] == mark[k] ? scn[k] : scenario_of_placement(h, starts, serial[k]);
    return IMGENV_OK;
}

// ---------------------------------------------------------------------------------------- step
// k_sfm for one step of every crowd, on stream s: from the live set into `out` (null: in place), with or without the write-back to
// the pedestrians' arrays
static int launch_sfm(imgenv* h, hipStream_t s, const SfmDev* out, int publish) {
    DevWorld d = h->d;
    if (out) sfm_write_into(d.sfm, *out);
    const int n_sfm = d.sfm.n, n_pairs = n_sfm * n_sfm;  // (of one world's crowd; a workgroup per world)
    const unsigned nw = (unsigned)h->W, pb = (unsigned)((n_pairs + SFM_MAX_AGENTS - 1) / SFM_MAX_AGENTS);
    if (n_pairs <= 4096) {  // small crowd: one launch
        TIMED(h, IMGENV_K_ORCA, s, (k_sfm<<<dim3(nw), dim3(SFM_MAX_AGENTS), sizeof(SfmNode) * SFM_LDS_NODES, s>>>(d, 0, publish)));
        h->launches += 1;
    } else {  // the n^2 pair terms (three correctly rounded atan2 each) spread over the chip between two one-workgroup launches
        const bool on = timing_on(h, IMGENV_K_ORCA);
        if (on) { if (int rc_ = timing_mark(h, IMGENV_K_ORCA, s, 0)) return rc_; }
        k_sfm<<<dim3(nw), dim3(SFM_MAX_AGENTS), sizeof(SfmNode) * SFM_LDS_NODES, s>>>(d, 1, publish);
        k_sfm<<<dim3(nw * pb), dim3(SFM_MAX_AGENTS), 0, s>>>(d, 2, publish);
        k_sfm<<<dim3(nw), dim3(SFM_MAX_AGENTS), sizeof(SfmNode) * SFM_LDS_NODES, s>>>(d, 3, publish);
        if (on) { if (int rc_ = timing_mark(h, IMGENV_K_ORCA, s, 1)) return rc_; }
        h->launches += 3;
    }
    return 0;
}
// Something is about to write the live crowd on stream st (a reset, a step in place, a device-side auto-reset): what was computed
// ahead is dropped, and the writer waits for the launch that may still be reading the live set
static int sfm_ahead_drop(imgenv* h, hipStream_t st) {
    if (h->crowd.valid) HIPCHK(hipStreamWaitEvent(st, h->crowd.ev, 0));
    h->crowd.valid = false;
    h->crowd.steps_since_reset = 0;
    return 0;
}

// the social-force crowd's step AHEAD, on its own stream (see imgenv_step_begin): queued once the step's own first kernels are out
static int sfm_launch_ahead(imgenv* h) {
    if (h->crowd.wait < 0) return 0;
    HIPCHK(hipStreamWaitEvent(h->crowd.stream, h->crowd.ev_in[h->crowd.wait], 0));
    h->crowd.wait = -1;
    if (int rc = launch_sfm(h, h->crowd.stream, &h->crowd.other, 0)) return rc;
    HIPCHK(hipEventRecord(h->crowd.ev, h->crowd.stream));
    h->crowd.valid = true;
    return 0;
}

// 1. Entry: what a step may not follow, the device's flags, the output guard; then the step's hand-over starts
static int step_entry(imgenv* h, const float* actions, hipStream_t st) {
    if (!h || !actions) FAIL(IMGENV_EINVAL, "null argument");
    if (!h->has_reset) FAIL(IMGENV_ESTATE, "step before reset");
    if (h->step.obs_forked) FAIL(IMGENV_ESTATE, "imgenv_step_begin twice without imgenv_step_end (reset the handle to recover from an aborted step)");
    RTRY(rollout_room(h));
    RTRY(check_device_flags(h));
    RTRY(outputs_verify(h, st));
    // (from here on the step's own kernels write output arrays; the chain's end seals them again.  A step that is begun and never
    // ended -- the caller's exchange failed -- must not read as "the caller wrote into imgenv_out" at the reset that recovers it)
    h->guard_sealed = false;
    h->step.actions = actions;
    h->launches = h->act.decode_launches;  // (imgenv_actions_decode in front of this step)
    h->act.decode_launches = 0;
    return 0;
}

// 2. PedScene::step + write-back (img_env.cpp:343-358) of a social-force crowd, as plan_crowd_step says (launch_plan.h has the
// ordering against the caller's stream).  A crowd that ignores the robots: this step's state was computed during the last step
// (sfm_launch_ahead) -- swap the two sets and publish -- or, right behind a reset, is computed now, in place; then the NEXT step's
// goes out on its stream, at the END of imgenv_step_begin, behind the step's own first launches (its five host calls in front of
// the move were ~25 us in which the caller's stream sat idle).
static int step_crowd(imgenv* h, hipStream_t st) {
    imgenv::CrowdAhead& c = h->crowd;
    if (!c.can) {  // a crowd that cannot run ahead steps in place and leaves nothing
        RTRY(sfm_ahead_drop(h, st));
        return launch_sfm(h, st, nullptr, 1);
    }
    const CrowdStep k = plan_crowd_step(c.can, c.valid, c.steps_since_reset, c.par);
    c.par = k.par_next;
    if (k.swap) {
        sfm_swap_sets(h->d.sfm, c.other);
        sfm_write_into(h->d.sfm, h->d.sfm);
        HIPCHK(hipStreamWaitEvent(st, c.ev, 0));
        // (the event rides on the kernel's dispatch packet: a hipEventRecord behind it is a packet of its own, ~6 us of the caller's stream)
        hipExtLaunchKernelGGL(k_sfm_publish, dim3((unsigned)h->W), dim3(SFM_MAX_AGENTS), 0, st, nullptr, c.ev_in[k.leaves], 0, h->d);
        h->launches += 1;
    } else {
        RTRY(launch_sfm(h, st, nullptr, 1));
        HIPCHK(hipEventRecord(c.ev_in[k.leaves], st));
    }
    c.wait = k.ahead_waits;
    c.steps_since_reset += 1;
    return 0;
}

// 4. _step_robot (img_env.cpp:388-410) in a launch of its own: k_integrate, the fork of the side streams right behind it on its
// dispatch packet, and in an early step the gate's number -- or its serial form where the sub-steps do not fit the LDS table
static int step_move(imgenv* h, const float* actions, hipStream_t st, const StepPlan& sp) {
    DevWorld& d = h->d;
    h->step.fork_on_move = sp.fork_on_move;
    if (!sp.serial_move)
        TIMED(h, IMGENV_K_INTEGRATE, st, (hipExtLaunchKernelGGL(k_integrate, dim3(sp.move.grid), dim3(sp.move.block), 0, st, nullptr,
                                                               sp.fork_on_move ? h->ev_fork : nullptr, 0, d, actions, sp.nb_robot, h->n_sub, h->elapsed,
                                                               sp.early_step ? h->step.gate_seq : 0u)));
    else
        TIMED(h, IMGENV_K_INTEGRATE, st, (k_integrate_serial<<<dim3(sp.move.grid), dim3(sp.move.block), 0, st>>>(d, actions, sp.nb_robot, h->elapsed)));
    return 0;
}

// 5. k_obs beside the move instead of behind it (world.h): it needs nothing of this step but the actions.  It waits behind a gate
// that opens when the caller's stream reaches the move (k_gate): everything queued there in front of the step is then complete
// -- whoever writes the actions, whoever still reads the last step's outputs, the last chain's views.  Queued BEHIND the move --
// a gate must follow the kernel that opens it in queue order; what the caller's stream forks behind the move is the solve alone.
static int early_obs(imgenv* h, const float* actions, hipStream_t st) {
    DevWorld& d = h->d;
    h->step.chain_open = true;
    if (!h->step.fork_on_move) HIPCHK(hipEventRecord(h->ev_fork, st));
    h->step.fork_on_move = false;
    k_gate<<<dim3(1), dim3(WAVE), 0, h->side2>>>(d.sync, h->step.gate_seq, d.err);
    h->launches += 1;
    d.obs_early = h->NA == 0 ? 2 : 1;  // (2: the pedestrians are live -- a social-force crowd a step ahead: see imgenv_create)
    d.obs_actions = actions; d.obs_n_sub = h->n_sub;
    d.ped_snap_in = h->ped_snap[plan_snap_in(h->step.orca_seq)];
    d.rec_snap_in = h->rec_snap[plan_snap_in(h->step.view_seq)];
    const int rc = launch_obs_kernel(h, h->side2, true);
    d.obs_early = 0;
    if (rc) return rc;
    h->step.obs_forked = true;
    h->step.early = true;
    return 0;
}

// The step up to the exchange: the crowd, the beep, the move in its three shapes (plan_step), the observation.  _step_ped_normal
// (img_env.cpp:304-359): the ORCA solve for this step ran on the side stream during the previous step's views and was joined at
// the end of that step; its velocities are applied by the move's pedestrian blocks.
extern "C" int imgenv_step_begin(imgenv_t* h, const float* actions, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    RTRY(step_entry(h, actions, st));
    DevWorld& d = h->d;
    if (h->cfg.ped_scene_type == IMGENV_SCENE_PEDSIM && d.sfm.n > 0) RTRY(step_crowd(h, st));
    if (d.beep_on) {  // 3. beep lottery + ERVO's evacuation term on top of the velocities the solve left (img_env.cpp:323-343)
        k_beep<<<dim3(h->W), dim3(BEEP_T), 0, st>>>(d, actions);
        k_evac<<<dim3(h->P), dim3(WAVE), 0, st>>>(d);
        h->launches += 2;
    }
    const StepPlan sp = plan_step(h->plan, chain_facts(h, 0));
    if (sp.early_step) h->step.gate_seq += 1;
    if (sp.sum_shard_now) {  // k_move_raster over the shard's own robots and the pedestrians, now (in front of the exchange)
        RTRY(launch_rasters(h, st, 0, true, true, true));
    } else if (sp.fuse_move) {  // k_move_raster, launched by launch_views (the fork of the side stream with it)
        h->step.move_pending = true;
        return sfm_launch_ahead(h);
    } else {
        RTRY(step_move(h, actions, st, sp));
    }
    h->launches += 1;
    set_tail_fields(h, 0, h->elapsed + 1);  // imgenv_step_end counts the step; k_obs goes out before that
    if (sp.early_step)
        RTRY(early_obs(h, actions, st));
    else if (h->P > 0)
        RTRY(launch_obs(h, st));
    // a robot shard in SUM mode (world.h: sum_shard) draws its own robots -- and the pedestrians -- NOW, in front of the exchange:
    // their records then carry the cells they cover to the other ranks
    if (d.sum_shard && !sp.sum_shard_now) RTRY(launch_rasters(h, st, 0, false, true, true));
    HIPCHK(hipGetLastError());
    return sfm_launch_ahead(h);
}

extern "C" int imgenv_step_end(imgenv_t* h, void* stream) {
    if (!h) FAIL(IMGENV_EINVAL, "null argument");
    if (!h->has_reset) FAIL(IMGENV_ESTATE, "step before reset");
    if (int rc = rollout_room(h)) return rc;
    h->elapsed += 1;  // TimeLimitWrapper._elapsed_steps (base.py:224)
    if (h->stamp) {  // this step's stamps get a new tag
        h->stamp_seq += 1;
        h->d.stamp_tag = h->stamp_seq % STAMP_TAGS + 1;
    }
    return launch_views(h, (hipStream_t)stream, 0);
}

extern "C" int imgenv_step(imgenv_t* h, const float* actions, void* stream) { return imgenv_step_flags(h, actions, 0u, stream); }

extern "C" int imgenv_step_flags(imgenv_t* h, const float* actions, uint32_t flags, void* stream) {
    (void)flags;  // (IMGENV_STEP_ACTIONS_READY: accepted, and since round 6 without effect -- include/imgenv.h)
    if (h) h->step.in_step = true;  // (begin and end in one call: the actions outlive the move whoever launches it)
    const int rc_begin = imgenv_step_begin(h, actions, stream);
    if (h) h->step.in_step = false;
    if (rc_begin) return rc_begin;
    if (h->comm) {  // the one exchange of a robot-sharded world: records of all robots, in place
        const size_t count = (size_t)h->RL * IMGENV_RECORD_DOUBLES;
        ncclResult_t e = ncclSuccess;
        TIMED(h, IMGENV_K_EXCHANGE, (hipStream_t)stream,
              e = rccl_api()->all_gather(h->d.rec + (size_t)h->r0 * IMGENV_RECORD_DOUBLES, h->d.rec, count, ncclDouble, h->comm, (hipStream_t)stream));
        if (e != ncclSuccess) FAIL(IMGENV_EDEVICE, "ncclAllGather: %s", rccl_api()->err(e));
    }
    return imgenv_step_end(h, stream);
}

// FNV-1a over everything spawn_world reads of a spawn cfg
static uint64_t spawn_cfg_fingerprint(const imgenv_spawn_cfg& c) {
    uint64_t hsh = 1469598103934665603ull;
    auto mix = [&](const void* p, size_t n) {
        const unsigned char* b = (const unsigned char*)p;
        for (size_t q = 0; q < n; q++) hsh = (hsh ^ b[q]) * 1099511628211ull;
    };
    mix(&c.n_robots, sizeof(int32_t) * 3);
    mix(&c.clearance, sizeof(double));
    mix(&c.target_min_dist, sizeof(double));
    mix(c.circle_ranges, sizeof(c.circle_ranges));
    mix(&c.go_back, sizeof(int32_t) * 2);
    for (int a = 0; a < c.n_robots + c.n_peds; a++) {
        const imgenv_spawn_agent& g = c.agents[a];
        mix(&g.begin_type, sizeof(int32_t) * 2);
        mix(g.begin, sizeof(g.begin));
        mix(g.target, sizeof(g.target));
        mix(&g.module_size, sizeof(double));
        mix(&g.n_begin_multi, sizeof(int32_t) * 2);
        if (g.begin_multi) mix(g.begin_multi, sizeof(double) * 6 * (size_t)g.n_begin_multi);
        if (g.target_multi) mix(g.target_multi, sizeof(double) * 6 * (size_t)g.n_target_multi);
    }
    for (int q = 0; q < c.n_obstacles; q++) {
        mix(&c.obstacles[q].shape, sizeof(int32_t) * 2);
        mix(c.obstacles[q].size_range, sizeof(c.obstacles[q].size_range));
        mix(c.obstacles[q].pose, sizeof(c.obstacles[q].pose));
    }
    return hsh;
}

// what both auto-reset calls ask of their arguments
static int autoreset_checks(imgenv* h, const float* actions, const imgenv_spawn_cfg* cfg, const char* who) {
    if (!h || !actions) FAIL(IMGENV_EINVAL, "null argument");
    if (int rc = spawn_cfg_check(cfg)) return rc;
    if (cfg->n_robots != h->Rw || cfg->n_peds != h->Pw)
        FAIL(IMGENV_EINVAL, "spawn cfg is for %d robots / %d pedestrians, a world of this handle has %d / %d", cfg->n_robots,
             cfg->n_peds, h->Rw, h->Pw);
    if (h->RL != h->R) FAIL(IMGENV_EINVAL, "%s needs all robots of every world on this handle", who);
    return rollout_room(h);
}

extern "C" int imgenv_step_autoreset(imgenv_t* h, const float* actions, const imgenv_spawn_cfg* cfg, uint64_t seed0, int32_t* worlds_out,
                                     int32_t cap, int32_t* n_out, void* stream) {
    if (!n_out) FAIL(IMGENV_EINVAL, "null argument");
    if (int rc = autoreset_checks(h, actions, cfg, "imgenv_step_autoreset")) return rc;
    *n_out = 0;
    const bool trace = imgenv::ResetTrace::on();  // where the host's time goes, every 200 calls
    double tp[5] = {0, 0, 0, 0, 0};
    if (trace) tp[0] = imgenv::ResetTrace::now_us();
    if (int rc = imgenv_step(h, actions, stream)) return rc;
    hipStream_t st = (hipStream_t)stream;
    k_finished<<<dim3(1), dim3(1024), 0, st>>>(h->d);
    if (int rc = outputs_seal(h, st)) return rc;  // (k_finished writes imgenv_out.step_all_down behind the step's own seal)
    HIPCHK(hipGetLastError());
    {   // while the device works: the placements of the next seeds (a placement depends on its seed alone, not on the world)
        const uint64_t fp = spawn_cfg_fingerprint(*cfg);
        if (fp != h->spawn_ahead_cfg) h->spawn_ahead.clear();
        h->spawn_ahead_cfg = fp;
        for (auto it = h->spawn_ahead.begin(); it != h->spawn_ahead.end();)  // seeds the caller has moved past
            it = (it->first - seed0 >= (uint64_t)h->spawn_ahead_n) ? h->spawn_ahead.erase(it) : std::next(it);
        for (int q = 0; q < h->spawn_ahead_n; q++) {
            std::unique_ptr<SpawnOut>& slot = h->spawn_ahead[seed0 + (uint64_t)q];
            if (slot) continue;
            slot.reset(new SpawnOut);
            if (spawn_world(*cfg, seed0 + (uint64_t)q, *slot)) slot->batch.struct_size = 0;  // could not be placed: reported if used
        }
    }
    if (trace) tp[1] = imgenv::ResetTrace::now_us();
    HIPCHK(hipStreamSynchronize(st));  // NeverStopWrapper reads the dones here too (base.py:205)
    if (trace) tp[2] = imgenv::ResetTrace::now_us();
    const int n = h->finished_host[0];
    if (n < 0 || n > h->W) FAIL(IMGENV_EDEVICE, "finished-world list is corrupt (%d)", n);
    int rc = IMGENV_OK;
    if (n > 0) {
        std::vector<int32_t> worlds((size_t)n);
        for (int q = 0; q < n; q++) worlds[q] = h->finished_host[1 + q];
        std::sort(worlds.begin(), worlds.end());  // the device lists them in no particular order; seeds go by ascending index
        // every placement first: a seed that cannot be placed fails the call BEFORE anything is handed out or taken from the
        // pre-drawn placements (the step itself has been applied; no world has been reset; *n_out stays 0; a repeated call
        // meets the same seeds)
        std::vector<SpawnOut*> use((size_t)n, nullptr);
        std::vector<std::unique_ptr<SpawnOut>> fresh;
        for (int q = 0; q < n; q++) {
            auto it = h->spawn_ahead.find(seed0 + (uint64_t)q);
            if (it != h->spawn_ahead.end() && it->second->batch.struct_size != 0) {
                use[q] = it->second.get();
            } else {
                fresh.emplace_back(new SpawnOut);
                if (const char* why = spawn_world(*cfg, seed0 + (uint64_t)q, *fresh.back()))
                    FAIL(IMGENV_EINVAL, "spawn of world %d (seed %llu): %s", worlds[q], (unsigned long long)(seed0 + (uint64_t)q), why);
                use[q] = fresh.back().get();
            }
        }
        std::vector<imgenv_reset_batch> batches((size_t)n);
        for (int q = 0; q < n; q++) batches[q] = use[q]->batch;
        h->spawn_ahead_n = std::min(256, std::max(8, 2 * n));  // twice what this step needed
        if (trace) tp[3] = imgenv::ResetTrace::now_us();
        const PlacementDraws draws = placement_draws(h, n, nullptr, seed0);  // the placement's seed also draws the map and the recorded crowd
        rc = reset_worlds(h, n, worlds.data(), batches.data(), draws.choices(), st);
        if (rc == IMGENV_OK) {
            *n_out = n;
            for (int q = 0; q < n && worlds_out && q < cap; q++) worlds_out[q] = worlds[q];
            for (int q = 0; q < n; q++) h->spawn_ahead.erase(seed0 + (uint64_t)q);  // consumed
        }
    } else if (trace) {
        tp[3] = imgenv::ResetTrace::now_us();
    }
    if (trace) {
        tp[4] = imgenv::ResetTrace::now_us();
        const double us[4] = {tp[1] - tp[0], tp[2] - tp[1], tp[3] - tp[2], tp[4] - tp[3]};
        imgenv::ResetTrace& tr = h->trace_autoreset;
        if (tr.add(us, 4, n))
            fprintf(stderr, "[imgenv_step_autoreset] %ld calls, %.1f worlds reset/call: step launches + placements ahead %.1f us, wait for the device %.1f us, "
                            "finished list %.1f us, reset launches %.1f us per call\n", tr.calls, (double)tr.worlds / tr.calls, tr.acc[0] / tr.calls,
                    tr.acc[1] / tr.calls, tr.acc[2] / tr.calls, tr.acc[3] / tr.calls);
    }
    return rc;
}


// ---------------------------------------------------------------------------------------- device-side auto-reset
// The pool's fill on the side stream, by the handle's scenario policy: the sampler (k_spawn_fill) or the bank (k_scenario_fill,
// the same launch shape: one wave64 workgroup per slot).  ev_fill says when it is done; the next chain waits for it in front of
// its k_respawn.
static int launch_pool_fill(imgenv* h, const SpawnDev& c) {
    if (h->scn_policy != IMGENV_SCENARIOS_OFF) {
        ScenarioSel b;
        b.agents = h->d_scn_agents; b.obst = h->d_scn_obst;
        b.n = h->n_scn; b.policy = h->scn_policy; b.first = (unsigned long long)h->scn_first;
        k_scenario_fill<<<dim3(c.S), dim3(WAVE), 0, h->dev.side3>>>(c, b);
    } else {
        k_spawn_fill<<<dim3(c.S), dim3(WAVE), 0, h->dev.side3>>>(c);
    }
    HIPCHK(hipEventRecord(h->dev.ev_fill, h->dev.side3));
    h->dev.fill_pending = true;
    return 0;
}

// The device arrays a pool owns besides its three cfg uploads, in allocation order: `each` gets the pointer, its element count and
// its fill byte.  Allocation and free both walk this list.
template <typename Each>
static int pool_arrays(SpawnDev& c, int W, Each&& each) {
    const size_t S = (size_t)c.S, na = (size_t)std::max(c.n_robots + c.n_peds, 1), nob = (size_t)std::max(c.n_obstacles, 1), Wz = (size_t)W;
    RTRY(each(c.slot_serial, S, 0xFF));
    RTRY(each(c.consumed, (size_t)2, 0));
    RTRY(each(c.slot_status, S, 0));
    RTRY(each(c.s_agents, S * na, 0));
    RTRY(each(c.s_obst, S * nob, 0));
    RTRY(each(c.s_inst, S * nob, 0));
    RTRY(each(c.s_rvo, S * c.cap_o, 0));
    RTRY(each(c.s_nodes, S * c.cap_n, 0));
    RTRY(each(c.s_rvo_n, S * 4, 0));
    RTRY(each(c.s_seg, S * nob * 4, 0));
    RTRY(each(c.fin_list, Wz, 0));
    RTRY(each(c.fin_n, (size_t)1, 0));
    RTRY(each(c.inst_out, Wz * nob, 0));
    RTRY(each(c.place_agents, Wz * na, 0));
    RTRY(each(c.place_obst, Wz * nob, 0));
    RTRY(each(c.place_serial, Wz, 0xFF));
    RTRY(each(c.w_inst, Wz * nob, 0));
    RTRY(each(c.w_inst_valid, Wz, 0));
    return 0;
}
// SpawnDev travels by value with every launch: its copies of the handle's pointers and strides are taken from the handle here,
// at set-up and whenever a host-side reset has re-laid a table (spawn_dev_refresh)
static void pool_aim(const imgenv* h, SpawnDev& c) {
    c.world_epoch = h->d_world_epoch;
    c.n_obst_w = h->d_wobst + 2 * (size_t)h->W;
    c.oroot_w = h->d_wobst + 3 * (size_t)h->W;
    c.w_obst = h->d_obst;
    c.w_nodes = h->d_nodes;
    c.traj = h->d_traj;
    c.traj_len = h->d_traj_len;
    c.traj_cap = h->traj_cap;
}
// another spawn cfg: the old pool goes (a curriculum that alternates cfgs would otherwise grow until imgenv_destroy)
static int pool_free(imgenv* h, hipStream_t st) {
    HIPCHK(hipStreamSynchronize(h->dev.side3));
    HIPCHK(hipStreamSynchronize(st));
    h->dev.ready = false;
    h->dev.fill_pending = false;
    SpawnDev o = h->dev.pool;
    DevSpawnAgent* oa = (DevSpawnAgent*)o.agents; DevSpawnObstacle* oo = (DevSpawnObstacle*)o.obstacles; double* om = (double*)o.multi;
    dev_free(h, oa); dev_free(h, oo); dev_free(h, om);
    return pool_arrays(o, h->W, [&](auto*& p, size_t, int) { return dev_free(h, p), 0; });
}
// the spawn cfg as the kernels read it, and the pool's own arrays (spawn_pool_check has passed)
static int pool_build(imgenv* h, const imgenv_spawn_cfg* cfg, uint64_t seed0) {
    SpawnDev& c = h->dev.pool;
    const int na = cfg->n_robots + cfg->n_peds, nob = cfg->n_obstacles;
    memset(&c, 0, sizeof(c));
    c.n_robots = cfg->n_robots; c.n_peds = cfg->n_peds; c.n_obstacles = nob; c.go_back = cfg->go_back; c.ignore_obstacle = cfg->ignore_obstacle;
    c.rvo = h->NA > 0 ? 1 : 0;
    c.sfm = h->cfg.ped_scene_type == IMGENV_SCENE_PEDSIM && h->d.sfm.n > 0 ? 1 : 0;
    c.clearance = cfg->clearance; c.target_min_dist = cfg->target_min_dist; c.circle0 = cfg->circle_ranges[0]; c.circle1 = cfg->circle_ranges[1];
    std::vector<DevSpawnAgent> ag((size_t)(na ? na : 1));
    std::vector<double> multi;
    for (int a = 0; a < na; a++) {
        const imgenv_spawn_agent& g = cfg->agents[a];
        DevSpawnAgent& o = ag[a];
        memset(&o, 0, sizeof(o));
        o.begin_type = g.begin_type; o.target_type = g.target_type; o.module_size = g.module_size;
        memcpy(o.begin, g.begin, sizeof(o.begin));
        memcpy(o.target, g.target, sizeof(o.target));
        if (g.begin_type == IMGENV_POSE_RANGE_MULTI) {
            o.begin_multi = (int)(multi.size() / 6); o.n_begin_multi = g.n_begin_multi;
            multi.insert(multi.end(), g.begin_multi, g.begin_multi + 6 * (size_t)g.n_begin_multi);
        }
        if (g.target_type == IMGENV_POSE_RANGE_MULTI) {
            o.target_multi = (int)(multi.size() / 6); o.n_target_multi = g.n_target_multi;
            multi.insert(multi.end(), g.target_multi, g.target_multi + 6 * (size_t)g.n_target_multi);
        }
    }
    if (multi.empty()) multi.push_back(0.0);
    std::vector<DevSpawnObstacle> ob((size_t)(nob ? nob : 1));
    for (int q = 0; q < nob; q++) {
        ob[q].shape = cfg->obstacles[q].shape; ob[q].pose_type = cfg->obstacles[q].pose_type;
        memcpy(ob[q].size_range, cfg->obstacles[q].size_range, sizeof(ob[q].size_range));
        memcpy(ob[q].pose, cfg->obstacles[q].pose, sizeof(ob[q].pose));
    }
    RTRY(dev_upload(h, &c.agents, ag));
    RTRY(dev_upload(h, &c.obstacles, ob));
    RTRY(dev_upload(h, &c.multi, multi));
    c.S = spawn_pool_slots(h->W);
    c.seed0 = seed0;
    c.cap_o = c.cap_n = spawn_slot_cap(nob);
    return pool_arrays(c, h->W, [&](auto*& p, size_t n, int fill) { return dev_alloc(h, &p, n, fill); });
}
// the per-world RVO tables take over from the host's copies: room for any placement's polygons in every world, and one stride for
// the worlds' slices and the slots'
static int pool_take_rvo(imgenv* h, hipStream_t st) {
    SpawnDev& c = h->dev.pool;
    const int W = h->W;
    if (h->NA > 0 && (h->cap_obst < c.cap_o || h->cap_nodes < c.cap_n)) {
        HIPCHK(hipStreamSynchronize(st));
        const int co = std::max(h->cap_obst, c.cap_o), cn = std::max(h->cap_nodes, c.cap_n);
        RvoObstDev* no = nullptr;
        RvoNodeDev* nn = nullptr;
        RTRY(dev_alloc(h, &no, (size_t)co * W));
        RTRY(dev_alloc(h, &nn, (size_t)cn * W));
        // every world's slice laid out on the host, then ONE copy per table (two blocking copies per world were 4 144 copies and
        // 21 ms for the 2048 envs of the shipped geometry)
        std::vector<RvoObstHost> all_o((size_t)co * W);
        std::vector<RvoNodeHost> all_n((size_t)cn * W);
        for (int q = 0; q < W; q++) {
            const RvoObstacles& rq = h->rvos[q];
            if ((int)rq.ob.size() > co || (int)rq.nodes.size() > cn) FAIL(IMGENV_ESTATE, "world %d holds more RVO obstacle vertices than a placement can have", q);
            std::copy(rq.ob.begin(), rq.ob.end(), all_o.begin() + (size_t)q * co);
            std::copy(rq.nodes.begin(), rq.nodes.end(), all_n.begin() + (size_t)q * cn);
            rvo_table_put(h->wobst, W, q, co, cn, rq);
        }
        HIPCHK(hipMemcpy(no, all_o.data(), sizeof(RvoObstDev) * all_o.size(), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(nn, all_n.data(), sizeof(RvoNodeDev) * all_n.size(), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(h->d_wobst, h->wobst.data(), sizeof(int) * h->wobst.size(), hipMemcpyHostToDevice));
        dev_free(h, h->d_obst);  // (st was synchronised above and every side stream is joined to it at the end of a step)
        dev_free(h, h->d_nodes);
        h->d_obst = no; h->d_nodes = nn; h->cap_obst = co; h->cap_nodes = cn;
        h->d.obst = no; h->d.onodes = nn;
    }
    if (h->NA > 0) {  // (slot arrays were sized with the smaller capacity: again with the handle's)
        c.cap_o = h->cap_obst;
        c.cap_n = h->cap_nodes;
        dev_free(h, c.s_rvo);
        dev_free(h, c.s_nodes);
        RTRY(dev_alloc(h, &c.s_rvo, (size_t)c.S * c.cap_o));
        RTRY(dev_alloc(h, &c.s_nodes, (size_t)c.S * c.cap_n));
    }
    return 0;
}
// check, free the old pool, build, take over the RVO tables, first fill
static int spawn_device_setup(imgenv* h, const imgenv_spawn_cfg* cfg, uint64_t seed0, hipStream_t st) {
    RTRY(spawn_pool_check(reset_facts(h), *cfg, g_err));
    const bool rebuilt = h->dev.ready;
    if (rebuilt) RTRY(pool_free(h, st));
    RTRY(pool_build(h, cfg, seed0));
    RTRY(pool_take_rvo(h, st));
    pool_aim(h, h->dev.pool);
    if (!h->dev.side3) {
        HIPCHK(hipStreamCreateWithFlags(&h->dev.side3, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&h->dev.ev_fill, hipEventDisableTiming | hipEventDisableSystemFence));
        HIPCHK(hipEventCreateWithFlags(&h->dev.ev_consumed, hipEventDisableTiming | hipEventDisableSystemFence));
    }
    HIPCHK(hipStreamSynchronize(st));  // (set-up only: the uploads above were synchronous copies)
    if (h->n_scn > 0 && rebuilt) {  // a new pool numbers its placements from 0 again: one epoch of the present policy, and no world's
        h->scn_epochs.assign(1, imgenv::ScnEpoch{h->scn_policy, h->scn_first});  // placement number means anything any more
        HIPCHK(hipMemset(h->d_scn_world, 0xFF, sizeof(int) * (size_t)h->W));
        HIPCHK(hipMemset(h->d_scn_mark, 0xFF, sizeof(unsigned long long) * (size_t)h->W));
    }
    RTRY(launch_pool_fill(h, h->dev.pool));  // (the next chain waits for this fill in front of its k_respawn, whatever fill_due says)
    h->dev.fill_due = 0;
    h->dev.ready = true;
    return 0;
}

// A host-side reset between two device-side steps may have re-laid the tables k_respawn writes into: reset_grow lays the
// trajectory table out again when a batch brings longer waypoint lists, and the per-world RVO slices (after imgenv_reset has
// handed them back to the host).  SpawnDev travels by value with every launch, so its copies of those pointers and strides are
// simply taken from the handle again; a changed RVO stride also moves the pool's slot arrays (slots and worlds share one
// stride), whose placements are then drawn again.
static int spawn_dev_refresh(imgenv* h, hipStream_t st) {
    SpawnDev& c = h->dev.pool;
    const bool stride = h->NA > 0 && (c.cap_o != h->cap_obst || c.cap_n != h->cap_nodes);
    const bool moved = c.traj != h->d_traj || c.traj_len != h->d_traj_len || c.traj_cap != h->traj_cap ||
                       (h->NA > 0 && (c.w_obst != h->d_obst || c.w_nodes != h->d_nodes));
    if (!stride && !moved) return 0;
    if (stride) {
        HIPCHK(hipStreamSynchronize(h->dev.side3));  // (a fill in flight writes the old slot arrays)
        HIPCHK(hipStreamSynchronize(st));
        c.cap_o = h->cap_obst;
        c.cap_n = h->cap_nodes;
        dev_free(h, c.s_rvo);  // (both streams are idle: nothing reads the old slot arrays any more)
        dev_free(h, c.s_nodes);
        RTRY(dev_alloc(h, &c.s_rvo, (size_t)c.S * c.cap_o));
        RTRY(dev_alloc(h, &c.s_nodes, (size_t)c.S * c.cap_n));
        HIPCHK(hipMemsetAsync(c.slot_serial, 0xFF, sizeof(unsigned long long) * (size_t)c.S, st));  // every slot is drawn again (the chain's own fill, behind this on st's event)
        h->dev.fill_due = 0;
    }
    pool_aim(h, c);
    return 0;
}

// one step + the reset of whatever it finished, everything queued on `st` and the handle's side streams (all joined again)
static int autoreset_device_chain(imgenv* h, const float* actions, hipStream_t st) {
    SpawnDev& c = h->dev.pool;
    DevWorld& d = h->d;
    const int W = h->W, nob = c.n_obstacles;
    // the pool, underneath the step: the slots whose placements earlier steps handed out -- on every SPAWN_FILL_PERIOD-th call
    // (two event operations and a launch less on the others: each costs the caller's stream a dependency bubble and the host a call)
    const bool fill = h->dev.fill_due <= 0;
    if (fill) {
        HIPCHK(hipEventRecord(h->dev.ev_consumed, st));
        HIPCHK(hipStreamWaitEvent(h->dev.side3, h->dev.ev_consumed, 0));
        RTRY(launch_pool_fill(h, c));
        h->dev.fill_due = SPAWN_FILL_PERIOD;
    }
    h->dev.fill_due -= 1;
    if (int rc = imgenv_step(h, actions, st)) return rc;
    k_finished_dev<<<dim3(1), dim3(1024), 0, st>>>(d, c);
    // (also the set-up's fill, which runs on the side stream whatever this call's fill_due was: k_respawn must not meet half-drawn slots)
    if (h->dev.fill_pending) HIPCHK(hipStreamWaitEvent(st, h->dev.ev_fill, 0));
    h->dev.fill_pending = false;
    const MapSel maps = map_sel(h);
    k_respawn<<<dim3(W), dim3(WAVE), 0, st>>>(d, c, h->elapsed, maps);
    if (h->d_trk_cur) {  // recorded crowds: every placed world takes its set of the bank (over the sampler's pedestrians, as init_ped_dataset does)
        const TracksPlan tp = plan_tracks_install(h->plan, 0, true, h->finished_host[0], h->trk_cap);
        k_tracks_install<<<dim3(tp.install.grid), dim3(tp.install.block), 0, st>>>(d, track_sel(h), c.fin_list, c.fin_n, 0, nullptr, c.place_serial, c.consumed,
                                                                                 (unsigned long long)c.seed0, h->d_traj, h->d_traj_v, h->d_traj_len, h->traj_cap);
        h->launches += 1;
    }
    // grids for a guess of the finished worlds (plan_dev_reset; the count is page-locked, written by k_finished_dev: stale by a step or two)
    const PlanHandle& p = h->plan;
    const DevResetPlan rp = plan_dev_reset(p, h->finished_host[0], nob);
    k_restore_maps_dev_for(p)<<<dim3(rp.restore.grid), dim3(rp.restore.block), 0, st>>>(d, c, h->d_static_map, maps, p.layer, rp.restore_blocks);
    if (nob > 0)
        k_reset_obstacles_for(p)<<<dim3(rp.obstacles.grid), dim3(rp.obstacles.block), 0, st>>>(d, c.inst_out, p.layer, c.fin_n, nob, rp.parts, c.w_inst, c.w_inst_valid);
    HIPCHK(hipGetLastError());
    if (h->stamp) {
        // The step's rasters have stamped the finished worlds' agents where they stood BEFORE the reset, with this step's tag,
        // and the map restore above only puts the obstacles' cells back: the reset's own rasters and views get a tag of their
        // own, under which those stamps have expired like any older ones (two tags per step; the sweep comes round accordingly)
        h->stamp_seq += 1;
        d.stamp_tag = h->stamp_seq % STAMP_TAGS + 1;
        if (h->stamp_seq % STAMP_TAGS == 0) k_cell_base<<<dim3(plan_compose_blocks(p, chain_facts(h, 1))), dim3(256), 0, st>>>(d);
    }
    // the launches behind: sized for every world, the list and its length read from device memory
    d.ptraj = h->d_traj;
    d.traj_cap = h->traj_cap;
    h->launches += 4;
    return with_active(h, c.fin_list, W, c.fin_n, [&] { return launch_views(h, st, 1); });
}

extern "C" int imgenv_step_autoreset_device(imgenv_t* h, const float* actions, const imgenv_spawn_cfg* cfg, uint64_t seed0, void* stream) {
    if (int rc = autoreset_checks(h, actions, cfg, "imgenv_step_autoreset_device")) return rc;
    if (!h->has_reset) FAIL(IMGENV_ESTATE, "step before reset");
    if (h->step.obs_forked) FAIL(IMGENV_ESTATE, "imgenv_step_autoreset_device between imgenv_step_begin and imgenv_step_end");
    hipStream_t st = (hipStream_t)stream;
    if (h->crowd.can) {  // kernels reset finished worlds here, crowds included, without the host knowing which: the crowd steps in place
        if (int rc = sfm_ahead_drop(h, st)) return rc;
        h->crowd.can = false;
    }
    if (h->scn_policy != IMGENV_SCENARIOS_OFF && (cfg->n_robots != h->Rw || cfg->n_peds != h->Pw || cfg->n_obstacles != h->scn_obst))
        FAIL(IMGENV_EINVAL, "imgenv_step_autoreset_device: the spawn cfg has %d robots / %d pedestrians / %d obstacles, the scenario bank %d / %d / %d",
             cfg->n_robots, cfg->n_peds, cfg->n_obstacles, h->Rw, h->Pw, h->scn_obst);
    const uint64_t fp = spawn_cfg_fingerprint(*cfg);
    if (!h->dev.ready || fp != h->dev.fp) {  // the first call fixes seed0: the k-th world reset from now on takes placement seed0 + k
        if (int rc = spawn_device_setup(h, cfg, seed0, st)) return rc;
        h->dev.fp = fp;
    }
    if (int rc = spawn_dev_refresh(h, st)) return rc;
    if (!h->d_act_list) RTRY(dev_alloc(h, &h->d_act_list, (size_t)h->W));
    h->dev.act_hint = plan_act_hint(h->plan, h->finished_host[0]);  // (page-locked, written by k_finished_dev; stale by a step or two: a hint only)
    const int rc = autoreset_device_chain(h, actions, st);
    if (rc == IMGENV_OK) h->dev.used = true;
    return rc;
}

// What the last imgenv_step_autoreset_device did (for checkers and hosts that want to know; synchronises `stream`): the worlds it
// reset, ascending (up to cap of them), their number, and the placement number the first of them took.
extern "C" int imgenv_autoreset_last(imgenv_t* h, int32_t* worlds_out, int32_t cap, int32_t* n_out, uint64_t* first_placement, void* stream) {
    if (!h || !n_out) FAIL(IMGENV_EINVAL, "null argument");
    if (!h->dev.ready) FAIL(IMGENV_ESTATE, "no imgenv_step_autoreset_device yet");
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    if (int rc = check_device_flags(h)) return rc;
    SpawnDev& c = h->dev.pool;
    const int n = h->finished_host[0];
    *n_out = n;
    for (int q = 0; q < n && worlds_out && q < cap; q++) worlds_out[q] = h->finished_host[1 + q];
    if (first_placement) {
        unsigned long long two[2];
        HIPCHK(hipMemcpy(two, c.consumed, sizeof(two), hipMemcpyDeviceToHost));
        *first_placement = two[1];
    }
    return IMGENV_OK;
}

// The placement world `world` currently runs, as its device-side reset received it (the arrays of imgenv_spawn(); any may be
// NULL), and its number.  Synchronises the device.
extern "C" int imgenv_world_placement(imgenv_t* h, int32_t world, uint64_t* placement, double* robot_pose, double* robot_goal, double* ped_pose,
                                      double* ped_goal, double* ped_traj, int32_t* ped_traj_len, int32_t* obs_shape, float* obs_size, double* obs_pose) {
    if (!h) FAIL(IMGENV_EINVAL, "null argument");
    if (!h->dev.ready) FAIL(IMGENV_ESTATE, "no imgenv_step_autoreset_device yet");
    if (world < 0 || world >= h->W) FAIL(IMGENV_EINVAL, "world out of range");
    HIPCHK(hipDeviceSynchronize());
    SpawnDev& c = h->dev.pool;
    const int nr = c.n_robots, np = c.n_peds, na = nr + np, nob = c.n_obstacles;
    unsigned long long serial = 0;
    HIPCHK(hipMemcpy(&serial, c.place_serial + world, sizeof(serial), hipMemcpyDeviceToHost));
    if (placement) *placement = serial;
    if (serial == ~0ull) FAIL(IMGENV_ESTATE, "world %d has not been reset by the device yet", world);
    std::vector<SlotAgent> ag((size_t)(na ? na : 1));
    std::vector<SlotObstacle> ob((size_t)(nob ? nob : 1));
    if (na) HIPCHK(hipMemcpy(ag.data(), c.place_agents + (size_t)world * na, sizeof(SlotAgent) * na, hipMemcpyDeviceToHost));
    if (nob) HIPCHK(hipMemcpy(ob.data(), c.place_obst + (size_t)world * nob, sizeof(SlotObstacle) * nob, hipMemcpyDeviceToHost));
    for (int i = 0; i < nr; i++) {
        if (robot_pose) { robot_pose[4 * i] = ag[i].x; robot_pose[4 * i + 1] = ag[i].y; robot_pose[4 * i + 2] = ag[i].qz; robot_pose[4 * i + 3] = ag[i].qw; }
        if (robot_goal) { robot_goal[2 * i] = ag[i].gx; robot_goal[2 * i + 1] = ag[i].gy; }
    }
    for (int j = 0; j < np; j++) {
        const SlotAgent& a = ag[nr + j];
        if (ped_pose) { ped_pose[4 * j] = a.x; ped_pose[4 * j + 1] = a.y; ped_pose[4 * j + 2] = a.qz; ped_pose[4 * j + 3] = a.qw; }
        if (ped_goal) { ped_goal[2 * j] = a.gx; ped_goal[2 * j + 1] = a.gy; }
        if (ped_traj) memcpy(ped_traj + 6 * (size_t)j, a.traj, sizeof(a.traj));
        if (ped_traj_len) ped_traj_len[j] = a.traj_len;
    }
    for (int q = 0; q < nob; q++) {
        if (obs_shape) obs_shape[q] = ob[q].shape;
        if (obs_size) memcpy(obs_size + 4 * (size_t)q, ob[q].size, sizeof(ob[q].size));
        if (obs_pose) { obs_pose[4 * q] = ob[q].x; obs_pose[4 * q + 1] = ob[q].y; obs_pose[4 * q + 2] = ob[q].qz; obs_pose[4 * q + 3] = ob[q].qw; }
    }
    return IMGENV_OK;
}

extern "C" int imgenv_comm_unique_id(void* id128) {
    if (!id128) FAIL(IMGENV_EINVAL, "null argument");
    RcclApi* a = rccl_api();
    if (!a) FAIL(IMGENV_EDEVICE, "RCCL (librccl.so) is not available");
    static_assert(sizeof(ncclUniqueId) == IMGENV_COMM_ID_BYTES, "ncclUniqueId size");
    const ncclResult_t e = a->get_id((ncclUniqueId*)id128);
    if (e != ncclSuccess) FAIL(IMGENV_EDEVICE, "ncclGetUniqueId: %s", a->err(e));
    return IMGENV_OK;
}

extern "C" int imgenv_comm_init(imgenv_t* h, const void* id128, int32_t rank, int32_t n_ranks) {
    if (!h || !id128 || n_ranks < 1 || rank < 0 || rank >= n_ranks) FAIL(IMGENV_EINVAL, "bad argument");
    RcclApi* a = rccl_api();
    if (!a) FAIL(IMGENV_EDEVICE, "RCCL (librccl.so) is not available");
    if (h->RL * n_ranks != h->R || h->r0 != rank * h->RL)
        FAIL(IMGENV_EINVAL, "native exchange needs equal contiguous shards: rank %d of %d owns [%d,%d) of %d robots", rank,
             n_ranks, h->r0, h->r1, h->R);
    HIPCHK(hipSetDevice(h->cfg.device));
    ncclUniqueId id;
    memcpy(&id, id128, sizeof(id));
    const ncclResult_t e = a->init_rank(&h->comm, n_ranks, id, rank);
    if (e != ncclSuccess) {
        h->comm = nullptr;
        FAIL(IMGENV_EDEVICE, "ncclCommInitRank: %s", a->err(e));
    }
    h->comm_ranks = n_ranks;
    return IMGENV_OK;
}

extern "C" int imgenv_comm_info(imgenv_t* h, int32_t* n_ranks, int32_t* rank) {
    if (!h) FAIL(IMGENV_EINVAL, "null argument");
    if (!h->comm) FAIL(IMGENV_ESTATE, "the handle has no communicator (imgenv_comm_init was not called)");
    int n = 0, r = 0;
    ncclResult_t e = rccl_api()->count(h->comm, &n);
    if (e == ncclSuccess) e = rccl_api()->user_rank(h->comm, &r);
    if (e != ncclSuccess) FAIL(IMGENV_EDEVICE, "ncclCommCount / ncclCommUserRank: %s", rccl_api()->err(e));
    if (n_ranks) *n_ranks = n;
    if (rank) *rank = r;
    return IMGENV_OK;
}

extern "C" int imgenv_records(imgenv_t* h, double** records, int64_t* bytes_per_robot) {
    if (!h) FAIL(IMGENV_EINVAL, "null argument");
    if (records) *records = h->d.rec;
    if (bytes_per_robot) *bytes_per_robot = IMGENV_RECORD_DOUBLES * (int64_t)sizeof(double);
    return IMGENV_OK;
}

extern "C" int imgenv_outputs(imgenv_t* h, imgenv_out* out) {
    if (!h || !out) FAIL(IMGENV_EINVAL, "null argument");
    // a caller built against an older, shorter imgenv_out says so in struct_size and gets no more than that many bytes
    // (fields are only ever appended); 0 = the caller's struct is this library's
    const int32_t want = out->struct_size;
    if (want < 0 || want > (int32_t)sizeof(imgenv_out)) FAIL(IMGENV_EINVAL, "imgenv_out.struct_size %d (this library's is %d)", want, (int)sizeof(imgenv_out));
    const imgenv_out& src = h->pub_arena ? h->pub_out : h->out;
    if (want == 0) {
        *out = src;
    } else {
        memcpy(out, &src, (size_t)want);
        out->struct_size = want;  // what the caller really holds, not this library's larger size
    }
    return IMGENV_OK;
}

// ---- what the enable / outputs entry points of the optional features share ----
// Every enable has one shape: feature_plan.h's X_enable_plan (the cfg's refusals, the null handle, the repeated call, the refusals
// that read the facts) -> the block's layout (launch_plan.h) -> ONE DevTxn -> fill dev and out -> enable_done.  Nothing of the
// handle changes before the transaction has committed.
// the facts the plan reads of this handle; nullptr for a null handle
static const FeatureFacts* feature_facts(const imgenv* h, FeatureFacts& f) {
    if (!h) return nullptr;
    f.RL = h->RL; f.P = h->P; f.state_dim = h->out.state_dim; f.ped_vec_dim = h->cfg.ped_vec_dim; f.n_beams = h->out.n_beams;
    f.keep_view_maps = h->d.keep_view_maps != 0;
    f.any_reset = any_world_reset(h);
    f.stack_on = h->stack.on; f.stack_state_depth = h->stack.out.state_depth; f.stack_n_fields = h->stack.dev.n_fields;
    f.ep_on = h->ep.on;
    f.eplog_on = h->eplog.on; f.eplog_capacity = h->eplog.dev.capacity;
    f.act_on = h->act.on; f.act_mode = h->act.cfg.mode; f.act_n_table = h->act.cfg.n_table; f.act_n_cols = h->act.cfg.n_cols;
    f.pol_on = h->pol.on; f.pol_kind = h->pol.cfg.kind; f.pol_flags = h->pol.cfg.flags; f.pol_A = h->pol.dev.A; f.pol_C = h->pol.dev.C;
    f.ploss_on = h->ploss.on;
    f.post_on = h->post.on; f.post_norm = h->post.dev.norm != nullptr;
    f.final_on = h->final_obs.on;
    f.roll_on = h->roll.on; f.roll_horizon = h->roll.cfg.horizon; f.roll_fields = h->roll.cfg.fields;
    f.mb_on = h->mb.on;
    f.seq_on = h->seq.on;
    f.norm_on = h->norm.on; f.norm_obs = h->norm.dev.norm_vector_states != nullptr; f.norm_rew = h->norm.dev.norm_rewards != nullptr;
    f.ped_h = h->cfg.ped_image_size[0]; f.ped_w = h->cfg.ped_image_size[1];
    return &f;
}
// what the plan decided, handed on: a refusal with its text; IMGENV_OK or ENABLE_REPEAT otherwise
static int planned(int rc, const FeatureMsg msg) {
    if (rc < 0) FAIL(rc, "%s", msg);
    return rc;
}
// an entry point that needs a feature: "imgenv_X_enable was not called"
static int needs(bool on, const char* enable_name) {
    FeatureMsg msg;
    return planned(feature_needed(on, enable_name, msg), msg);
}
// the same cfg again: the stored out struct, nothing changes
template <typename F, typename Out>
static int enable_repeated(const F& f, Out* out) {
    if (out) *out = f.out;
    return IMGENV_OK;
}
// (imgenv_episode_log_out and imgenv_policy_loss_out have no n_local)
template <typename Out, typename = void>
struct HasNLocal : std::false_type {};
template <typename Out>
struct HasNLocal<Out, std::void_t<decltype(Out::n_local)>> : std::true_type {};
// the end of an enable call: `o`, zeroed but for the feature's own fields, becomes the handle's struct and the feature is on
template <typename F, typename Out>
static int enable_done(imgenv* h, F& f, Out o, Out* out) {
    o.struct_size = (int32_t)sizeof(Out);
    if constexpr (HasNLocal<Out>::value) o.n_local = h->RL;
    f.out = o;
    f.on = true;
    if (out) *out = o;
    return IMGENV_OK;
}
// a feature's one block (launch_plan.h has the layouts): `total` zeroed bytes that the handle owns from here on
static int feature_block(imgenv* h, size_t total, const char* enable_name, unsigned char** block) {
    HIPCHK(hipSetDevice(h->cfg.device));
    DevTxn<HipApi> txn;
    if (!txn.room(block, total, 0)) FAIL(txn.code(), "%s: %s", enable_name, txn.error());
    txn.commit(h->allocs);
    return IMGENV_OK;
}
template <typename F, typename Out>
static int feature_outputs(imgenv* h, F imgenv::*feature, Out* out, const char* enable_name) {
    if (!h || !out) FAIL(IMGENV_EINVAL, "null argument");
    RTRY(needs((h->*feature).on, enable_name));
    *out = (h->*feature).out;
    return IMGENV_OK;
}

// ---- observation stacks (include/imgenv.h; the kernel is csrc/stack.h) ----
static StackPlan stack_plan(const imgenv_cfg& c, const imgenv_stack_cfg& s, int RL) {
    return plan_stack((size_t)c.image_size[0] * (size_t)c.image_size[1], c.state_dim, make_view_geom(c).B, s.image_batch, s.state_batch, s.laser_batch, (size_t)RL);
}

extern "C" int64_t imgenv_stack_bytes(const imgenv_cfg* cfg, const imgenv_stack_cfg* s) {
    if (!cfg || !s) FAIL(IMGENV_EINVAL, "null argument");
    if (cfg->struct_size != (int32_t)sizeof(imgenv_cfg) || s->struct_size != (int32_t)sizeof(imgenv_stack_cfg)) FAIL(IMGENV_EINVAL, "struct_size mismatch");
    int r0, r1;
    if (shard_of(*cfg, r0, r1)) FAIL(IMGENV_EINVAL, "bad robot shard");
    FeatureMsg msg;
    if (int rc = planned(stack_cfg_refusals(*s, msg), msg)) return rc;
    return (int64_t)stack_plan(*cfg, *s, r1 - r0).total;
}

extern "C" int imgenv_stack_enable(imgenv_t* h, const imgenv_stack_cfg* s, imgenv_stack_out* out) {
    FeatureMsg msg;
    FeatureFacts facts;
    RTRY(planned(stack_enable_plan(s, out, feature_facts(h, facts), msg), msg));
    const StackPlan p = stack_plan(h->cfg, *s, h->RL);
    if (p.total > 0 && s->arena) RTRY(planned(stack_arena_refusals(*s, p.total, msg), msg));
    HIPCHK(hipSetDevice(h->cfg.device));
    unsigned char* base = nullptr;
    if (p.total > 0) {
        if (s->arena) {
            base = (unsigned char*)s->arena;
            HIPCHK(hipMemset(base, 0, p.total));
        } else {
            RTRY(feature_block(h, p.total, "imgenv_stack_enable", &base));
        }
    }
    const imgenv_out& pub = h->pub_arena ? h->pub_out : h->out;
    unsigned char* const work[3] = {(unsigned char*)h->out.sensor_maps, (unsigned char*)h->out.vector_states, (unsigned char*)h->out.lasers};
    unsigned char* const handed[3] = {(unsigned char*)pub.sensor_maps, (unsigned char*)pub.vector_states, (unsigned char*)pub.lasers};
    unsigned char* ptr[3] = {nullptr, nullptr, nullptr};
    StackDev sd;
    memset(&sd, 0, sizeof(sd));
    for (int k = 0; k < 3; k++) {
        if (p.depth[k] == 1) ptr[k] = handed[k];  // [R][1][...] is the imgenv_out array itself
        if (p.depth[k] < 2) continue;
        ptr[k] = base + p.off[k];
        StackField& f = sd.f[sd.n_fields++];
        f.stack = ptr[k];
        f.frame = work[k];
        // (a frame is whole float16, float32 or float64 words: its size is even, and the rule never answers the unit 1 k_stack leaves out)
        const FinalFieldPlan fp = plan_final_field(p.frame_bytes[k]);
        f.frame_bytes = fp.row_bytes;
        f.unit = fp.unit;
        f.chunks = fp.chunks;
        f.depth = p.depth[k];
        sd.chunks_per_robot += f.chunks;
    }
    h->stack.dev = sd;
    imgenv_stack_out o = {};
    o.image_depth = p.depth[0]; o.state_depth = p.depth[1]; o.laser_depth = p.depth[2];
    o.sensor_maps = (uint16_t*)ptr[0]; o.vector_states = (float*)ptr[1]; o.lasers = (double*)ptr[2];
    return enable_done(h, h->stack, o, out);
}

// the chain's tail (launch_tails): a step pushes every local robot's new frames, a reset chain restarts the stacks of the robots it covers
static void tail_stack(imgenv* h, hipStream_t st, const ChainPlans& k) {
    if (!h->stack.on || h->stack.dev.n_fields <= 0) return;
    StackDev sd = h->stack.dev;
    sd.rows = tail_rows(h, k.is_reset);
    const LaunchShape g = plan_tail_launch(h->plan, k.c, sd.chunks_per_robot, STACK_BLOCK, STACK_MAX_BLOCKS);
    (k.is_reset ? k_stack<true> : k_stack<false>)<<<dim3(g.grid), dim3(g.block), 0, st>>>(sd);
    h->launches += 1;
}

extern "C" int imgenv_stack_outputs(imgenv_t* h, imgenv_stack_out* out) {
    return feature_outputs(h, &imgenv::stack, out, "imgenv_stack_enable");
}

// ---- episode statistics (include/imgenv.h; the kernel is csrc/episodes.h) ----
static_assert(EPF_OPEN_ROWS == IMGENV_EP_OPEN_F64 && EPI_EPISODES - EPI_ENDS0 == IMGENV_EP_END_BINS && EPF_RETURN_SUM - EPF_FIG0 == IMGENV_EP_FIGURES,
              "episodes.h rows against include/imgenv.h");
extern "C" int imgenv_episodes_enable(imgenv_t* h, const imgenv_episodes_cfg* c, imgenv_episodes_out* out) {
    FeatureMsg msg;
    FeatureFacts facts;
    const int plan = planned(episodes_enable_plan(c, out, feature_facts(h, facts), h ? &h->ep.cfg : nullptr, msg), msg);
    if (plan) return plan < 0 ? plan : enable_repeated(h->ep, out);
    const size_t RL = (size_t)h->RL, f_bytes = sizeof(double) * EPF_ROWS * RL, i_bytes = sizeof(int32_t) * EPI_ROWS * RL;
    unsigned char* base = nullptr;
    RTRY(feature_block(h, f_bytes + i_bytes, "imgenv_episodes_enable", &base));  // (zeroed: no episode open)
    EpisodesDev e;
    memset(&e, 0, sizeof(e));
    e.f = (double*)base;
    e.i = (int32_t*)(base + f_bytes);
    e.step_rewards = h->out.step_rewards;  // (the working arena, also under IMGENV_FLAG_FULL_REWRITE)
    e.step_is_clean = h->out.step_is_clean;
    e.step_dones_info = h->out.step_dones_info;
    e.dt = c->dt;
    e.min_steps = c->min_steps;
    h->ep.dev = e;
    h->ep.cfg = *c;
    h->ep.clear_bytes = f_bytes + sizeof(int32_t) * EPI_CLEARED_ROWS * RL;
    imgenv_episodes_out o = {};
    o.ends = e.i + EPI_ENDS0 * RL; o.episodes = e.i + EPI_EPISODES * RL; o.short_episodes = e.i + EPI_SHORT * RL;
    o.speed_steps = e.i + EPI_SPEED_STEPS * RL; o.arrive_steps = e.i + EPI_ARRIVE_STEPS * RL; o.len_sum = e.i + EPI_LEN_SUM * RL;
    o.v_sum = e.f + EPF_V_SUM * RL; o.w_sum = e.f + EPF_W_SUM * RL; o.figure_sums = e.f + EPF_FIG0 * RL; o.return_sum = e.f + EPF_RETURN_SUM * RL;
    o.last_code = e.i + EPI_LAST_CODE * RL; o.last_steps = e.i + EPI_LAST_STEPS * RL; o.last_len = e.i + EPI_LAST_LEN * RL;
    o.last_episode = e.i + EPI_LAST_EPISODE * RL; o.last_return = e.f + EPF_LAST_RETURN * RL;
    o.open_f64 = e.f; o.open_steps = e.i + EPI_TMP_STEPS * RL; o.open_len = e.i + EPI_LEN * RL; o.open = e.i + EPI_OPEN * RL;
    return enable_done(h, h->ep, o, out);
}

// the chain's tail (launch_tails): a step's command, reward and is_clean go into every local robot's open episode, a reset chain
// folds the episodes of the robots it covers by the last step's dones_info.  In front of that fold the episode log
// (episode_log.h): one record per episode this chain closes, and the tags of the episodes it opens -- from the words the chain's
// earlier launches have written (the banks' pointers are taken here: they may have come, or been rebuilt, after the log's enable)
static void tail_episodes(imgenv* h, hipStream_t st, const ChainPlans& k) {
    if (!h->ep.on) return;
    EpisodesDev ed = h->ep.dev;
    ed.actions = h->step.actions;
    ed.rows = tail_rows(h, k.is_reset);
    if (k.is_reset && h->eplog.on) {
        EpisodeLogDev lg = h->eplog.dev;
        lg.map_cur = h->d_map_cur; lg.trk_cur = h->d_trk_cur; lg.scn_world = h->d_scn_world; lg.scn_mark = h->d_scn_mark;
        lg.place_serial = h->dev.ready ? h->dev.pool.place_serial : nullptr;
        const LaunchShape gl = plan_episode_log_launch();
        k_episode_log<<<dim3(gl.grid), dim3(gl.block), 0, st>>>(ed, lg);
        h->launches += 1;
    }
    const LaunchShape g = plan_tail_launch(h->plan, k.c, 1, EP_BLOCK, EP_MAX_BLOCKS);
    (k.is_reset ? k_episodes<true> : k_episodes<false>)<<<dim3(g.grid), dim3(g.block), 0, st>>>(ed);
    h->launches += 1;
}

extern "C" int imgenv_episodes_outputs(imgenv_t* h, imgenv_episodes_out* out) {
    return feature_outputs(h, &imgenv::ep, out, "imgenv_episodes_enable");
}

extern "C" int imgenv_episodes_clear(imgenv_t* h, void* stream) {
    if (!h) FAIL(IMGENV_EINVAL, "null argument");
    RTRY(needs(h->ep.on, "imgenv_episodes_enable"));
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipMemsetAsync(h->ep.dev.f, 0, h->ep.clear_bytes, (hipStream_t)stream));
    return IMGENV_OK;
}

// ---- episode log (include/imgenv.h; the kernel is csrc/episode_log.h) ----
static_assert(EPL_I32_ROWS == IMGENV_EPLOG_I32 && EPL_F64_ROWS == IMGENV_EPLOG_F64 && EPLOG_SCN_DEVICE == IMGENV_EPLOG_SCN_DEVICE &&
                  sizeof(imgenv_episode_record) == 128,
              "episode_log.h rows against include/imgenv.h");
extern "C" int imgenv_episode_log_enable(imgenv_t* h, const imgenv_episode_log_cfg* c, imgenv_episode_log_out* out) {
    FeatureMsg msg;
    FeatureFacts facts;
    const int plan = planned(episode_log_enable_plan(c, out, feature_facts(h, facts), msg), msg);
    if (plan) return plan < 0 ? plan : enable_repeated(h->eplog, out);
    HIPCHK(hipSetDevice(h->cfg.device));
    // two blocks: the counter and the ring's placement | f64 | i32 columns, zeroed; the per-robot tags (placement | i32), which start
    // as "open before the log was" (all bits set: -1 and ~0).  Nothing of the handle changes before both are there.
    const size_t C = (size_t)c->capacity, RL = (size_t)h->RL;
    const size_t ring_bytes = 8 + C * (8 + 8 * EPL_F64_ROWS + 4 * EPL_I32_ROWS), tag_bytes = RL * (8 + 4 * EPT_ROWS);
    unsigned char *b = nullptr, *t = nullptr;
    DevTxn<HipApi> txn;
    txn.room(&b, ring_bytes, 0);
    txn.room(&t, tag_bytes, 0xFF);
    if (txn.code()) FAIL(txn.code(), "imgenv_episode_log_enable: a log of %d records: %s", c->capacity, txn.error());
    txn.commit(h->allocs);
    EpisodeLogDev g;
    memset(&g, 0, sizeof(g));
    g.n_written = (unsigned long long*)b;
    g.placement = (unsigned long long*)(b + 8);
    g.f64 = (double*)(b + 8 + 8 * C);
    g.i32 = (int32_t*)(b + 8 + 8 * C + 8 * EPL_F64_ROWS * C);
    g.tag_place = (unsigned long long*)t;
    g.tags = (int32_t*)(t + 8 * RL);
    g.capacity = c->capacity;
    g.W = h->W;
    h->eplog.dev = g;
    imgenv_episode_log_out o = {};
    o.capacity = c->capacity;
    o.n_written = (uint64_t*)g.n_written; o.i32 = g.i32; o.f64 = g.f64; o.placement = (uint64_t*)g.placement;
    return enable_done(h, h->eplog, o, out);
}

extern "C" int imgenv_episode_log_outputs(imgenv_t* h, imgenv_episode_log_out* out) {
    return feature_outputs(h, &imgenv::eplog, out, "imgenv_episode_log_enable");
}

extern "C" int64_t imgenv_episode_log_read(imgenv_t* h, uint64_t first, int32_t max, imgenv_episode_record* rec, uint64_t* oldest, uint64_t* n_written,
                                           void* stream) {
    if (!h || max < 0 || (max > 0 && !rec)) FAIL(IMGENV_EINVAL, "null argument");
    RTRY(needs(h->eplog.on, "imgenv_episode_log_enable"));
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    if (int rc = check_device_flags(h)) return rc;
    const EpisodeLogDev& g = h->eplog.dev;
    const uint64_t C = (uint64_t)g.capacity;
    unsigned long long n = 0;
    HIPCHK(hipMemcpy(&n, g.n_written, sizeof(n), hipMemcpyDeviceToHost));
    const uint64_t old = n > C ? n - C : 0;
    if (oldest) *oldest = old;
    if (n_written) *n_written = n;
    const uint64_t lo = std::max(first, old), want_end = first + (uint64_t)max, hi = want_end < first ? n : std::min<uint64_t>(want_end, n);
    if (lo >= hi) return 0;
    const size_t cnt = (size_t)(hi - lo);
    // the slots of [lo, hi): one or two runs of the ring, column by column
    std::vector<int32_t> ci(cnt * EPL_I32_ROWS);
    std::vector<double> cf(cnt * EPL_F64_ROWS);
    std::vector<unsigned long long> cp(cnt);
    const size_t s0 = (size_t)(lo % C), run0 = std::min(cnt, (size_t)C - s0), run1 = cnt - run0;
    auto pull = [&](void* dst, const void* col, size_t elem) -> hipError_t {
        hipError_t e = hipMemcpy(dst, (const unsigned char*)col + s0 * elem, run0 * elem, hipMemcpyDeviceToHost);
        if (e == hipSuccess && run1) e = hipMemcpy((unsigned char*)dst + run0 * elem, col, run1 * elem, hipMemcpyDeviceToHost);
        return e;
    };
    for (int k = 0; k < EPL_I32_ROWS; k++) HIPCHK(pull(ci.data() + (size_t)k * cnt, g.i32 + (size_t)k * C, 4));
    for (int k = 0; k < EPL_F64_ROWS; k++) HIPCHK(pull(cf.data() + (size_t)k * cnt, g.f64 + (size_t)k * C, 8));
    HIPCHK(pull(cp.data(), g.placement, 8));
    // the scenario of a device-placed episode: its placement number under the policy of the epoch it falls into (imgenv_world_scenarios)
    std::vector<unsigned long long> starts;
    if (h->n_scn > 0) RTRY(scenario_starts_pull(h, starts));
    for (size_t q = 0; q < cnt; q++) {
        imgenv_episode_record& r = rec[q];
        const int32_t* i = ci.data() + q;
        r.seq = lo + q;
        r.placement = cp[q];
        r.robot = i[EPL_ROBOT * cnt]; r.world = i[EPL_WORLD * cnt]; r.code = i[EPL_CODE * cnt]; r.steps = i[EPL_STEPS * cnt];
        r.len = i[EPL_LEN * cnt]; r.counted = i[EPL_COUNTED * cnt]; r.episode = i[EPL_EPISODE * cnt]; r.map = i[EPL_MAP * cnt];
        r.tracks = i[EPL_TRACKS * cnt];
        int32_t scn = i[EPL_SCENARIO * cnt];
        if (h->n_scn < 1) scn = -1;
        else if (scn == IMGENV_EPLOG_SCN_DEVICE) scn = scenario_of_placement(h, starts, cp[q]);
        r.scenario = scn;
        r.ep_return = cf[EPL_RETURN * cnt + q];
        for (int k = 0; k < 8; k++) r.figures[k] = cf[(EPL_FIG0 + k) * cnt + q];
    }
    return (int64_t)cnt;
}

// ---- action decoding (include/imgenv.h; the kernel is csrc/actions.h) ----
extern "C" int imgenv_actions_enable(imgenv_t* h, const imgenv_actions_cfg* c, imgenv_actions_out* out) {
    FeatureMsg msg;
    FeatureFacts facts;
    const int plan = planned(actions_enable_plan(c, out, feature_facts(h, facts), h ? &h->act.cfg : nullptr, h ? h->act.table.data() : nullptr, msg), msg);
    if (plan) return plan < 0 ? plan : enable_repeated(h->act, out);
    HIPCHK(hipSetDevice(h->cfg.device));
    const size_t RL = (size_t)h->RL;
    ActionsDev a;
    memset(&a, 0, sizeof(a));
    // three zeroed arrays and, in TABLE mode, the rows: one transaction, nothing of the handle changes before all are there
    std::vector<float> table;
    float* d_table = nullptr;
    DevTxn<HipApi> txn;
    txn.room(&a.actions, RL * 3, 0);
    txn.room(&a.speeds, RL * 2, 0);
    txn.room(&a.n_bad, 1, 0);
    if (c->mode == IMGENV_ACTIONS_TABLE) {
        table.assign(c->table, c->table + 3 * (size_t)c->n_table);
        txn.room(&d_table, table.size(), 0);
        txn.put(d_table, table.data(), sizeof(float) * table.size());
        a.n_table = c->n_table;
    } else {
        for (int i = 0; i < c->n_cols; i++) { a.lo[i] = c->clip[i][0]; a.hi[i] = c->clip[i][1]; }
    }
    if (txn.code()) FAIL(txn.code(), "imgenv_actions_enable: %s", txn.error());
    txn.commit(h->allocs);
    a.table = d_table;
    a.clean_state = h->d.clean_state;
    a.n_cols = c->n_cols;
    a.RL = h->RL;
    h->act.dev = a;
    h->act.cfg = *c;
    h->act.cfg.table = nullptr;
    h->act.table.swap(table);
    imgenv_actions_out o = {};
    o.actions = a.actions; o.speeds = a.speeds; o.n_bad = a.n_bad;
    return enable_done(h, h->act, o, out);
}

extern "C" int imgenv_actions_outputs(imgenv_t* h, imgenv_actions_out* out) {
    return feature_outputs(h, &imgenv::act, out, "imgenv_actions_enable");
}

// k_actions<DTYPE, MODE>: the six instantiations (indices are not clipped)
typedef void (*ActionsKernel)(const ActionsDev);
static ActionsKernel k_actions_for(int dtype, int mode) {
    if (mode == IMGENV_ACTIONS_CLIP) return dtype == IMGENV_RAW_F32 ? k_actions<IMGENV_RAW_F32, IMGENV_ACTIONS_CLIP> : k_actions<IMGENV_RAW_F64, IMGENV_ACTIONS_CLIP>;
    switch (dtype) {
        case IMGENV_RAW_I32: return k_actions<IMGENV_RAW_I32, IMGENV_ACTIONS_TABLE>;
        case IMGENV_RAW_I64: return k_actions<IMGENV_RAW_I64, IMGENV_ACTIONS_TABLE>;
        case IMGENV_RAW_F32: return k_actions<IMGENV_RAW_F32, IMGENV_ACTIONS_TABLE>;
        default: return k_actions<IMGENV_RAW_F64, IMGENV_ACTIONS_TABLE>;
    }
}
extern "C" int imgenv_actions_decode(imgenv_t* h, const void* raw, int32_t dtype, void* stream) {
    if (!h || !raw) FAIL(IMGENV_EINVAL, "null argument");
    RTRY(needs(h->act.on, "imgenv_actions_enable"));
    if (!h->has_reset) FAIL(IMGENV_ESTATE, "imgenv_actions_decode before the first reset");
    if (dtype < IMGENV_RAW_I32 || dtype > IMGENV_RAW_F64) FAIL(IMGENV_EINVAL, "imgenv_actions_decode: dtype %d", dtype);
    const bool integer = dtype == IMGENV_RAW_I32 || dtype == IMGENV_RAW_I64;
    if (integer && h->act.cfg.mode == IMGENV_ACTIONS_CLIP) FAIL(IMGENV_EINVAL, "imgenv_actions_decode: indices in CLIP mode (the handle has no table)");
    const size_t elem = dtype == IMGENV_RAW_I32 || dtype == IMGENV_RAW_F32 ? 4 : 8;
    if ((uintptr_t)raw % elem != 0) FAIL(IMGENV_EINVAL, "imgenv_actions_decode: raw is not aligned to its %d-byte elements", (int)elem);
    HIPCHK(hipSetDevice(h->cfg.device));
    ActionsDev a = h->act.dev;
    a.raw = raw;
    const LaunchShape g = plan_actions_launch(h->plan);
    k_actions_for(dtype, h->act.cfg.mode)<<<dim3(g.grid), dim3(g.block), 0, (hipStream_t)stream>>>(a);
    HIPCHK(hipGetLastError());
    h->act.decode_launches += 1;
    return IMGENV_OK;
}

// ---- the policy head (include/imgenv.h; the kernels are csrc/policy.h) ----
extern "C" int imgenv_policy_enable(imgenv_t* h, const imgenv_policy_cfg* c, imgenv_policy_out* out) {
    FeatureMsg msg;
    FeatureFacts facts;
    const int plan = planned(policy_enable_plan(c, out, feature_facts(h, facts), h ? &h->pol.cfg : nullptr, msg), msg);
    if (plan) return plan < 0 ? plan : enable_repeated(h->pol, out);
    const bool cat = c->kind == IMGENV_POLICY_CATEGORICAL, store = (c->flags & IMGENV_POLICY_STORE) != 0;
    const size_t RL = (size_t)h->RL, T = store ? (size_t)facts.roll_horizon : 0;
    const int n_params = cat ? facts.act_n_table : facts.act_n_cols;
    const PolicyLayout l = plan_policy_layout(cat, cat ? 1 : (size_t)n_params, RL, T);
    unsigned char* block = nullptr;
    RTRY(feature_block(h, l.total, "imgenv_policy_enable", &block));
    imgenv_policy_out o = {};
    o.n_params = n_params;
    o.horizon = (int32_t)T;
    if (cat) o.index = (int32_t*)(block + l.index);
    else o.raw = (float*)(block + l.raw);
    o.logp = (float*)(block + l.logp);
    o.entropy = (float*)(block + l.entropy);
    if (store) {
        o.pol_raw = (float*)(block + l.pol_raw);
        o.pol_logp = (float*)(block + l.pol_logp);
        o.pol_value = (float*)(block + l.pol_value);
    }
    PolicyDev p;
    memset(&p, 0, sizeof(p));
    const ActionsDev& a = h->act.dev;
    p.table = a.table; p.actions = a.actions; p.speeds = a.speeds; p.n_bad = a.n_bad; p.clean_state = a.clean_state;
    for (int i = 0; i < 3; i++) { p.lo[i] = a.lo[i]; p.hi[i] = a.hi[i]; }
    p.index = o.index; p.raw = o.raw; p.logp = o.logp; p.entropy = o.entropy;
    p.st_col = T * RL;
    p.g0 = (unsigned long long)h->r0;
    p.seed_lo = (uint32_t)c->seed; p.seed_hi = (uint32_t)(c->seed >> 32);
    p.A = cat ? n_params : 0; p.C = cat ? 0 : n_params; p.RL = h->RL;
    h->pol.dev = p;
    h->pol.cfg = *c;
    return enable_done(h, h->pol, o, out);
}

extern "C" int imgenv_policy_outputs(imgenv_t* h, imgenv_policy_out* out) {
    return feature_outputs(h, &imgenv::pol, out, "imgenv_policy_enable");
}

typedef void (*PolicyKernel)(const PolicyDev);
static PolicyKernel k_policy_cat_for(int G) {
    PolicyKernel k = nullptr;
    pick([&](auto g) { k = k_policy_cat<decltype(g)::value>; }, OneOf<1, 4, 16, 64>{G});
    return k;
}
extern "C" int imgenv_policy_sample(imgenv_t* h, const imgenv_policy_args* g, void* stream) {
    if (!h || !g) FAIL(IMGENV_EINVAL, "null argument");
    if (g->struct_size != (int32_t)sizeof(imgenv_policy_args)) FAIL(IMGENV_EINVAL, "imgenv_policy_args.struct_size %d (this library's is %d)", g->struct_size, (int)sizeof(imgenv_policy_args));
    const int32_t known = IMGENV_POLICY_DETERMINISTIC | IMGENV_POLICY_LOG_STD_PER_ROW | IMGENV_POLICY_NO_STORE | IMGENV_POLICY_VALUE_ONLY;
    if (g->flags & ~known) FAIL(IMGENV_EINVAL, "imgenv_policy_args.flags %d", g->flags);
    RTRY(needs(h->pol.on, "imgenv_policy_enable"));
    if (!h->has_reset) FAIL(IMGENV_ESTATE, "imgenv_policy_sample before the first reset");
    const bool cat = h->pol.cfg.kind == IMGENV_POLICY_CATEGORICAL, value_only = (g->flags & IMGENV_POLICY_VALUE_ONLY) != 0;
    const bool stores = (h->pol.cfg.flags & IMGENV_POLICY_STORE) && !(g->flags & IMGENV_POLICY_NO_STORE);
    auto misaligned = [](const void* p) { return (uintptr_t)p % 4 != 0; };
    if (value_only) {
        if (g->flags != IMGENV_POLICY_VALUE_ONLY) FAIL(IMGENV_EINVAL, "imgenv_policy_args.flags %d: IMGENV_POLICY_VALUE_ONLY stands alone", g->flags);
        if (!(h->pol.cfg.flags & IMGENV_POLICY_STORE)) FAIL(IMGENV_ESTATE, "imgenv_policy_sample: IMGENV_POLICY_VALUE_ONLY on a head without IMGENV_POLICY_STORE");
        if (!g->values || misaligned(g->values)) FAIL(IMGENV_EINVAL, "imgenv_policy_args.values is null or misaligned");
    } else {
        if (!g->params || misaligned(g->params)) FAIL(IMGENV_EINVAL, "imgenv_policy_args.params is null or misaligned");
        if (!cat && (!g->log_std || misaligned(g->log_std))) FAIL(IMGENV_EINVAL, "imgenv_policy_args.log_std is null or misaligned");
        if (cat && (g->flags & IMGENV_POLICY_LOG_STD_PER_ROW)) FAIL(IMGENV_EINVAL, "imgenv_policy_args.flags: IMGENV_POLICY_LOG_STD_PER_ROW on a categorical head");
        if (g->values && misaligned(g->values)) FAIL(IMGENV_EINVAL, "imgenv_policy_args.values is misaligned");
    }
    PolicyDev p = h->pol.dev;
    if (stores || value_only) {
        // the slot: the rollout cursor as the host holds it (the state the window's next transition starts from)
        const int n = h->roll.begun ? h->roll.n : -1, T = h->roll.cfg.horizon;
        if (n < 0 || n > T || (n == T && !value_only))
            FAIL(IMGENV_ESTATE, "imgenv_policy_sample: slot %d of a window of %d (imgenv_rollout_begin starts the next one)", n, T);
        const size_t at = (size_t)n * (size_t)h->RL;
        if (!value_only) { p.st_raw = h->pol.out.pol_raw + at; p.st_logp = h->pol.out.pol_logp + at; }
        p.st_value = h->pol.out.pol_value + at;
    }
    p.params = g->params; p.log_std = g->log_std; p.values = g->values;
    p.draw_lo = (uint32_t)g->draw; p.draw_hi = (uint32_t)(g->draw >> 32);
    p.det = (g->flags & IMGENV_POLICY_DETERMINISTIC) ? 1 : 0;
    p.ls_per_row = (g->flags & IMGENV_POLICY_LOG_STD_PER_ROW) ? 1 : 0;
    HIPCHK(hipSetDevice(h->cfg.device));
    const LaunchShape s = plan_policy_launch(h->plan, value_only ? 0 : p.A);
    const PolicyKernel k = value_only ? k_policy_value : cat ? k_policy_cat_for(plan_policy_group(p.A)) : k_policy_gauss;
    k<<<dim3(s.grid), dim3(s.block), 0, (hipStream_t)stream>>>(p);
    HIPCHK(hipGetLastError());
    if (!value_only) h->act.decode_launches += 1;  // (the values-only call belongs to no step)
    return IMGENV_OK;
}

// ---- PPO's loss (include/imgenv.h; the kernels are csrc/policy_loss.h) ----
extern "C" int imgenv_policy_loss_enable(imgenv_t* h, const imgenv_policy_loss_cfg* c, imgenv_policy_loss_out* out) {
    FeatureMsg msg;
    FeatureFacts facts;
    const int plan = planned(policy_loss_enable_plan(c, out, feature_facts(h, facts), h ? &h->ploss.cfg : nullptr, msg), msg);
    if (plan) return plan < 0 ? plan : enable_repeated(h->ploss, out);
    const bool cat = facts.pol_kind == IMGENV_POLICY_CATEGORICAL;
    const size_t n = (size_t)(cat ? facts.pol_A : facts.pol_C);
    const size_t n_rec = plan_policy_loss_launch(c->max_rows, cat ? facts.pol_A : 0).grid;
    const PolicyLossLayout l = plan_policy_loss_layout(cat, (size_t)c->max_rows, n, n_rec, PLOSS_REC);
    unsigned char* block = nullptr;
    RTRY(feature_block(h, l.total, "imgenv_policy_loss_enable", &block));
    imgenv_policy_loss_out o = {};
    o.n_params = (int32_t)n;
    o.max_rows = c->max_rows;
    o.logp = (float*)(block + l.logp); o.entropy = (float*)(block + l.entropy); o.ratio = (float*)(block + l.ratio);
    o.pg = (float*)(block + l.pg); o.vl = (float*)(block + l.vl);
    o.d_params = (float*)(block + l.d_params);
    if (!cat) { o.d_log_std = (float*)(block + l.d_log_std); o.d_log_std_shared = (float*)(block + l.d_log_std_shared); }
    o.d_values = (float*)(block + l.d_values);
    o.stats = (float*)(block + l.stats); o.n_bad = (int32_t*)(block + l.n_bad); o.inv_w = (float*)(block + l.inv_w);
    PlossDev p;
    memset(&p, 0, sizeof(p));
    p.logp = o.logp; p.entropy = o.entropy; p.ratio = o.ratio; p.pg = o.pg; p.vl = o.vl;
    p.d_params = o.d_params; p.d_log_std = o.d_log_std; p.d_log_std_shared = o.d_log_std_shared; p.d_values = o.d_values;
    p.stats = o.stats; p.n_bad = o.n_bad; p.inv_W = o.inv_w;
    if (cat) { p.row_m = (float*)(block + l.row_m); p.row_log_s = (float*)(block + l.row_log_s); }
    p.row_gu = (float*)(block + l.row_gu); p.row_w = (float*)(block + l.row_w);
    p.rec = (double*)(block + l.rec);
    p.A = facts.pol_A; p.C = facts.pol_C;
    h->ploss.dev = p;
    h->ploss.cfg = *c;
    return enable_done(h, h->ploss, o, out);
}

extern "C" int imgenv_policy_loss_outputs(imgenv_t* h, imgenv_policy_loss_out* out) {
    return feature_outputs(h, &imgenv::ploss, out, "imgenv_policy_loss_enable");
}

typedef void (*PlossKernel)(const PlossDev);
static void k_ploss_cat_for(int G, PlossKernel& rows, PlossKernel& grad) {
    pick([&](auto g) { rows = k_ploss_cat<decltype(g)::value>; grad = k_ploss_grad_cat<decltype(g)::value>; }, OneOf<1, 4, 16, 64>{G});
}
extern "C" int imgenv_policy_loss(imgenv_t* h, const imgenv_policy_loss_args* g, void* stream) {
    if (!h || !g) FAIL(IMGENV_EINVAL, "null argument");
    if (g->struct_size != (int32_t)sizeof(imgenv_policy_loss_args)) FAIL(IMGENV_EINVAL, "imgenv_policy_loss_args.struct_size %d (this library's is %d)", g->struct_size, (int)sizeof(imgenv_policy_loss_args));
    if (g->flags & ~(IMGENV_PLOSS_CLIP_VALUE | IMGENV_POLICY_LOG_STD_PER_ROW)) FAIL(IMGENV_EINVAL, "imgenv_policy_loss_args.flags %d", g->flags);
    if (g->reserved != 0) FAIL(IMGENV_EINVAL, "imgenv_policy_loss_args.reserved %d", g->reserved);
    RTRY(needs(h->ploss.on, "imgenv_policy_loss_enable"));
    if (g->rows < 1 || g->rows > h->ploss.cfg.max_rows) FAIL(IMGENV_EINVAL, "imgenv_policy_loss_args.rows %d (1 .. %d)", g->rows, h->ploss.cfg.max_rows);
    const bool cat = h->pol.cfg.kind == IMGENV_POLICY_CATEGORICAL, clip_value = (g->flags & IMGENV_PLOSS_CLIP_VALUE) != 0;
    if (cat && (g->flags & IMGENV_POLICY_LOG_STD_PER_ROW)) FAIL(IMGENV_EINVAL, "imgenv_policy_loss_args.flags: IMGENV_POLICY_LOG_STD_PER_ROW on a categorical head");
    auto missing = [](const void* p) { return !p || (uintptr_t)p % 4 != 0; };
    if (missing(g->params) || missing(g->values) || missing(g->old_logp) || missing(g->adv) || missing(g->ret) || missing(g->weight))
        FAIL(IMGENV_EINVAL, "imgenv_policy_loss_args: params, values, old_logp, adv, ret or weight is null or misaligned");
    if (!cat && missing(g->log_std)) FAIL(IMGENV_EINVAL, "imgenv_policy_loss_args.log_std is null or misaligned");
    if (clip_value && missing(g->old_value)) FAIL(IMGENV_EINVAL, "imgenv_policy_loss_args.old_value is null or misaligned");
    for (int c = 0; c < (cat ? 1 : h->ploss.dev.C); c++)
        if (missing(g->action[c])) FAIL(IMGENV_EINVAL, "imgenv_policy_loss_args.action[%d] is null or misaligned", c);
    if (!(g->clip >= 0.0f)) FAIL(IMGENV_EINVAL, "imgenv_policy_loss_args.clip %g", (double)g->clip);
    if (clip_value && !(g->clip_vf >= 0.0f)) FAIL(IMGENV_EINVAL, "imgenv_policy_loss_args.clip_vf %g", (double)g->clip_vf);
    PlossDev p = h->ploss.dev;
    p.params = g->params; p.log_std = g->log_std; p.values = g->values;
    for (int c = 0; c < 3; c++) p.action[c] = g->action[c];
    p.old_logp = g->old_logp; p.old_value = g->old_value; p.adv = g->adv; p.ret = g->ret; p.weight = g->weight;
    p.clip = g->clip; p.clip_vf = g->clip_vf; p.vf_coef = g->vf_coef; p.ent_coef = g->ent_coef;
    p.B = g->rows;
    p.clip_value = clip_value ? 1 : 0;
    p.ls_per_row = (g->flags & IMGENV_POLICY_LOG_STD_PER_ROW) ? 1 : 0;
    const LaunchShape s = plan_policy_loss_launch(p.B, cat ? p.A : 0);
    p.n_rec = (int32_t)s.grid;
    PlossKernel rows = k_ploss_gauss, grad = k_ploss_grad_gauss;
    if (cat) k_ploss_cat_for(plan_policy_group(p.A), rows, grad);
    HIPCHK(hipSetDevice(h->cfg.device));
    const hipStream_t st = (hipStream_t)stream;
    rows<<<dim3(s.grid), dim3(s.block), 0, st>>>(p);
    k_ploss_fold<<<dim3(1), dim3(PLOSS_FOLD_BLOCK), 0, st>>>(p);
    grad<<<dim3(s.grid), dim3(s.block), 0, st>>>(p);
    HIPCHK(hipGetLastError());
    return IMGENV_OK;
}

// ---- observation post-processing (include/imgenv.h; the kernel is csrc/obs_post.h) ----
extern "C" int imgenv_obs_post_enable(imgenv_t* h, const imgenv_obs_post_cfg* c, imgenv_obs_post_out* out) {
    FeatureMsg msg;
    FeatureFacts facts;
    const int plan = planned(obs_post_enable_plan(c, out, feature_facts(h, facts), h ? &h->post.cfg : nullptr, msg), msg);
    if (plan) return plan < 0 ? plan : enable_repeated(h->post, out);
    HIPCHK(hipSetDevice(h->cfg.device));
    ObsPostDev p;
    memset(&p, 0, sizeof(p));
    p.flags = c->flags;
    p.PV = h->d.PV;
    p.max_ped = h->cfg.max_ped;
    p.per_row = (c->flags & IMGENV_OBS_PED_NORM) ? p.PV : 1;
    p.ped_vector_states = h->out.ped_vector_states;  // (the working arena, also under IMGENV_FLAG_FULL_REWRITE)
    p.ped_min_dists = h->out.ped_min_dists;
    // one zeroed array per flag, in one transaction: nothing of the handle changes before both are there
    DevTxn<HipApi> txn;
    if (c->flags & IMGENV_OBS_PED_NORM) {
        txn.room(&p.norm, (size_t)h->RL * p.PV, 0);
        for (int k = 0; k < OBS_POST_DIM; k++) { p.avg[k] = c->avg[k]; p.std[k] = c->std[k]; }
    }
    if (c->flags & IMGENV_OBS_CLOSE) {
        txn.room(&p.close, (size_t)h->RL, 0);
        p.close_dist = c->close_dist;
    }
    if (txn.code()) FAIL(txn.code(), "imgenv_obs_post_enable: %s", txn.error());
    txn.commit(h->allocs);
    h->post.dev = p;
    h->post.cfg = *c;
    imgenv_obs_post_out o = {};
    o.ped_vector_norm = p.norm;
    o.close_to_human = p.close;
    return enable_done(h, h->post, o, out);
}

// the chain's tail (launch_tails): the normalised pedestrian vectors and close_to_human of every local robot after a step, of the
// robots a reset chain covers
static void tail_obs_post(imgenv* h, hipStream_t st, const ChainPlans& k) {
    if (!h->post.on) return;
    ObsPostDev pd = h->post.dev;
    pd.rows = tail_rows(h, k.is_reset);
    const LaunchShape g = plan_tail_launch(h->plan, k.c, (size_t)pd.per_row, OBS_POST_BLOCK, OBS_POST_MAX_BLOCKS);
    (k.is_reset ? k_obs_post<true> : k_obs_post<false>)<<<dim3(g.grid), dim3(g.block), 0, st>>>(pd);
    h->launches += 1;
}

extern "C" int imgenv_obs_post_outputs(imgenv_t* h, imgenv_obs_post_out* out) {
    return feature_outputs(h, &imgenv::post, out, "imgenv_obs_post_enable");
}

// ---- running normalisation (include/imgenv.h; the kernels are csrc/normalise.h) ----
extern "C" int imgenv_normalise_enable(imgenv_t* h, const imgenv_normalise_cfg* c, imgenv_normalise_out* out) {
    FeatureMsg msg;
    FeatureFacts facts;
    RTRY(planned(normalise_enable_plan(c, out, feature_facts(h, facts), msg), msg));
    const imgenv_out& w = h->out;
    const imgenv_stack_out& so = h->stack.out;
    const int D = facts.state_dim;
    const bool obs = (c->flags & IMGENV_NORM_OBS) != 0, rew = (c->flags & IMGENV_NORM_REWARD) != 0;
    const int K = normalise_stack_depth(facts, obs);
    // one block with the initial statistics in it; nothing of the handle changes before it is there
    const size_t words = NORM_STATS_WORDS(D);
    const NormaliseLayout l = plan_normalise_layout((size_t)h->RL, D, K, obs, rew);
    HIPCHK(hipSetDevice(h->cfg.device));
    unsigned char* block = nullptr;
    DevTxn<HipApi> txn;
    if (!txn.room(&block, l.total, 0)) FAIL(txn.code(), "imgenv_normalise_enable: %s", txn.error());
    std::vector<double> init(2 * words, 0.0);  // SB3's RunningMeanStd: count 1e-4, mean 0, var 1 -- in both words
    for (int q = 0; q < 2; q++) {
        double* s = init.data() + q * words;
        s[0] = s[1] = 1e-4;
        s[3] = 1.0;
        for (int d = 0; d < D; d++) s[4 + D + d] = 1.0;
    }
    if (const char* e = HipApi::memcpy(block + l.stats, init.data(), init.size() * 8, false)) FAIL(IMGENV_EDEVICE, "imgenv_normalise_enable: %s", e);
    txn.commit(h->allocs);
    NormDev n;
    memset(&n, 0, sizeof(n));
    n.vector_states = w.vector_states;  // (the working arena, also under IMGENV_FLAG_FULL_REWRITE)
    n.state_stack = K ? so.vector_states : nullptr;
    n.rewards = w.step_rewards;
    n.is_clean = w.step_is_clean;
    n.dones = w.step_dones;
    n.stats = (double*)(block + l.stats);
    n.returns = rew ? (double*)(block + l.returns) : nullptr;
    n.part = (double*)(block + l.part);
    n.part_n = (uint32_t*)(block + l.part_n);
    n.norm_vector_states = obs ? (float*)(block + l.norm_vector_states) : nullptr;
    n.norm_state_stack = K ? (float*)(block + l.norm_state_stack) : nullptr;
    n.norm_rewards = rew ? (double*)(block + l.norm_rewards) : nullptr;
    n.gamma = c->gamma; n.clip_obs = c->clip_obs; n.clip_reward = c->clip_reward; n.eps = c->eps;
    n.D = D;
    n.K = K;
    n.n_obs = obs ? D : 0;
    h->norm.dev = n;
    h->norm.cfg = *c;
    h->norm.training = true;
    h->norm.turn = h->norm.ret_turn = 0;
    imgenv_normalise_out o = {};
    o.state_dim = D;
    o.state_depth = K;
    o.norm_vector_states = n.norm_vector_states;
    o.norm_state_stack = n.norm_state_stack;
    o.norm_rewards = n.norm_rewards;
    o.stats = n.stats;
    o.returns = n.returns;
    o.training = 1;
    return enable_done(h, h->norm, o, out);
}

// the chain's tail (launch_tails): what plan_norm_chain says of this chain -- the batch into the statistics, the statistics onto the rows
static void tail_normalise(imgenv* h, hipStream_t st, const ChainPlans& k) {
    if (!h->norm.on) return;
    NormDev nd = h->norm.dev;
    const NormChain n = plan_norm_chain(h->norm.training, (h->norm.cfg.flags & IMGENV_NORM_REWARD) != 0, nd.n_obs, k.is_reset != 0);
    nd.rows = tail_rows(h, k.is_reset);
    nd.n_ret = n.n_ret; nd.cols = n.cols; nd.update = n.update;
    nd.turn = h->norm.turn; nd.ret_turn = h->norm.ret_turn;
    if (n.part) {
        const LaunchShape g = plan_norm_part_launch(h->plan, k.c, nd.cols);
        (k.is_reset ? k_norm_part<true> : k_norm_part<false>)<<<dim3(g.grid), dim3(g.block), 0, st>>>(nd);
        h->launches += 1;
    }
    if (n.apply) {
        const LaunchShape g = plan_norm_apply_launch(h->plan, k.c, nd.cols);
        (k.is_reset ? k_norm_apply<true> : k_norm_apply<false>)<<<dim3(g.grid), dim3(g.block), 0, st>>>(nd);
        h->launches += 1;
    }
    if (n.turn) h->norm.turn += 1;
    if (n.ret_turn) h->norm.ret_turn += 1;
}

extern "C" int imgenv_normalise_outputs(imgenv_t* h, imgenv_normalise_out* out) {
    if (int rc = feature_outputs(h, &imgenv::norm, out, "imgenv_normalise_enable")) return rc;
    out->stats_word = (int32_t)(h->norm.turn & 1);
    out->returns_word = (int32_t)(h->norm.ret_turn & 1);
    out->training = h->norm.training ? 1 : 0;
    return IMGENV_OK;
}

extern "C" int imgenv_normalise_training(imgenv_t* h, int32_t on, void* stream) {
    (void)stream;  // (a host-side switch: the chains queued from now on take it by value)
    if (!h) FAIL(IMGENV_EINVAL, "null argument");
    RTRY(needs(h->norm.on, "imgenv_normalise_enable"));
    h->norm.training = on != 0;
    return IMGENV_OK;
}

static int normalise_stats_args(const imgenv* h, const imgenv_normalise_stats* s) {
    if (!h || !s) FAIL(IMGENV_EINVAL, "null argument");
    if (s->struct_size != (int32_t)sizeof(imgenv_normalise_stats)) FAIL(IMGENV_EINVAL, "imgenv_normalise_stats.struct_size %d (this library's is %d)", s->struct_size, (int)sizeof(imgenv_normalise_stats));
    RTRY(needs(h->norm.on, "imgenv_normalise_enable"));
    if (s->state_dim != h->norm.dev.D || s->n_rows != h->RL) FAIL(IMGENV_EINVAL, "imgenv_normalise_stats: state_dim %d, n_rows %d (the handle's are %d, %d)", s->state_dim, s->n_rows, h->norm.dev.D, h->RL);
    if (!s->obs_mean || !s->obs_var) FAIL(IMGENV_EINVAL, "imgenv_normalise_stats: null obs_mean / obs_var");
    return IMGENV_OK;
}

extern "C" int imgenv_normalise_stats_get(imgenv_t* h, imgenv_normalise_stats* s) {
    RTRY(normalise_stats_args(h, s));
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipDeviceSynchronize());
    const size_t D = (size_t)h->norm.dev.D, words = NORM_STATS_WORDS(D), RL = (size_t)h->RL;
    std::vector<double> host(words);
    HIPCHK(hipMemcpy(host.data(), h->norm.dev.stats + (size_t)(h->norm.turn & 1) * words, words * 8, hipMemcpyDeviceToHost));
    s->obs_count = host[0]; s->ret_count = host[1]; s->ret_mean = host[2]; s->ret_var = host[3];
    for (size_t d = 0; d < D; d++) {
        s->obs_mean[d] = host[4 + d];
        s->obs_var[d] = host[4 + D + d];
    }
    if (s->returns) {
        if (h->norm.dev.returns)
            HIPCHK(hipMemcpy(s->returns, h->norm.dev.returns + (size_t)(h->norm.ret_turn & 1) * RL, RL * 8, hipMemcpyDeviceToHost));
        else
            std::fill(s->returns, s->returns + RL, 0.0);
    }
    return IMGENV_OK;
}

extern "C" int imgenv_normalise_stats_set(imgenv_t* h, const imgenv_normalise_stats* s) {
    RTRY(normalise_stats_args(h, s));
    const size_t D = (size_t)h->norm.dev.D, words = NORM_STATS_WORDS(D), RL = (size_t)h->RL;
    std::vector<double> host(words);
    host[0] = s->obs_count; host[1] = s->ret_count; host[2] = s->ret_mean; host[3] = s->ret_var;
    for (size_t d = 0; d < D; d++) {
        host[4 + d] = s->obs_mean[d];
        host[4 + D + d] = s->obs_var[d];
    }
    for (size_t k = 0; k < words; k++)
        if (!std::isfinite(host[k])) FAIL(IMGENV_EINVAL, "imgenv_normalise_stats: word %d is not finite", (int)k);
    if (host[0] <= 0.0 || host[1] <= 0.0) FAIL(IMGENV_EINVAL, "imgenv_normalise_stats: a count of %g / %g (above 0)", host[0], host[1]);
    if (host[3] < 0.0) FAIL(IMGENV_EINVAL, "imgenv_normalise_stats.ret_var %g", host[3]);
    for (size_t d = 0; d < D; d++)
        if (host[4 + D + d] < 0.0) FAIL(IMGENV_EINVAL, "imgenv_normalise_stats.obs_var[%d] %g", (int)d, host[4 + D + d]);
    if (s->returns)
        for (size_t r = 0; r < RL; r++)
            if (!std::isfinite(s->returns[r])) FAIL(IMGENV_EINVAL, "imgenv_normalise_stats.returns[%d] is not finite", (int)r);
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(h->norm.dev.stats + (size_t)(h->norm.turn & 1) * words, host.data(), words * 8, hipMemcpyHostToDevice));
    if (s->returns && h->norm.dev.returns)
        HIPCHK(hipMemcpy(h->norm.dev.returns + (size_t)(h->norm.ret_turn & 1) * RL, s->returns, RL * 8, hipMemcpyHostToDevice));
    HIPCHK(hipDeviceSynchronize());
    return IMGENV_OK;
}

// ---- the fields a feature can copy rows of (csrc/obs_fields.h) ----
// the catalogue of this handle: the sources are always in the working arena
static void handle_obs_fields(const imgenv* h, ObsField (&f)[OBSF_COUNT]) {
    ObsFacts a = {};
    a.out = h->out;
    a.ped_image_size[0] = h->cfg.ped_image_size[0];
    a.ped_image_size[1] = h->cfg.ped_image_size[1];
    a.stack = h->stack.out;
    a.ped_vector_norm = h->post.dev.norm;
    if (h->norm.on) {  // (normalise.h's arrays; the stack only where the handle keeps one)
        a.norm_vector_states = h->norm.dev.norm_vector_states;
        a.norm_state_stack = h->norm.dev.norm_state_stack;
        a.norm_K = h->norm.dev.K;
    }
    obs_fields(a, f);
}

// ---- final observations (include/imgenv.h; the kernel is csrc/final_obs.h) ----
extern "C" int imgenv_final_obs_enable(imgenv_t* h, const imgenv_final_obs_cfg* c, imgenv_final_obs_out* out) {
    FeatureMsg msg;
    FeatureFacts facts;
    const int plan_rc = planned(final_obs_enable_plan(c, out, feature_facts(h, facts), h ? &h->final_obs.cfg : nullptr, msg), msg);
    if (plan_rc) return plan_rc < 0 ? plan_rc : enable_repeated(h->final_obs, out);
    ObsField fields[OBSF_COUNT];
    handle_obs_fields(h, fields);
    FieldSelection s;
    RTRY(planned(select_feature_fields(FIELDS_FINAL, fields, c->fields, c->fields, s, msg), msg));
    const FinalPlan plan = plan_final_fields(s.row_bytes, s.n);
    // one zeroed block (launch_plan.h).  Nothing of the handle changes before it is there.
    const FinalObsLayout l = plan_final_obs_layout(s.row_bytes, s.n, (size_t)h->RL);
    unsigned char* block = nullptr;
    RTRY(feature_block(h, l.total, "imgenv_final_obs_enable", &block));
    imgenv_final_obs_out o = {};
    FinalObsDev fo;
    memset(&fo, 0, sizeof(fo));
    fo.n_fields = plan.n_fields;
    fo.chunks_per_row = plan.chunks_per_row;
    fo.count = (uint32_t*)(block + l.count);
    for (int k = 0; k < s.n; k++) {
        const ObsSlot& slot = OBS_SLOTS[s.id[k]];
        fo.f[k].dst = block + l.field[k];
        fo.f[k].src = (const unsigned char*)fields[s.id[k]].src;
        fo.f[k].unit = plan.f[k].unit;
        fo.f[k].chunks = plan.f[k].chunks;
        obs_slot_put(slot, slot.final_out, &o, &h->norm.out, fo.f[k].dst);
    }
    o.final_count = fo.count;
    h->final_obs.dev = fo;
    h->final_obs.cfg = *c;
    return enable_done(h, h->final_obs, o, out);
}

extern "C" int imgenv_final_obs_outputs(imgenv_t* h, imgenv_final_obs_out* out) {
    return feature_outputs(h, &imgenv::final_obs, out, "imgenv_final_obs_enable");
}

// ---- rollout storage (include/imgenv.h; the kernels are csrc/rollout.h) ----
extern "C" int imgenv_rollout_enable(imgenv_t* h, const imgenv_rollout_cfg* c, imgenv_rollout_out* out) {
    FeatureMsg msg;
    FeatureFacts facts;
    const int plan = planned(rollout_enable_plan(c, out, feature_facts(h, facts), h ? &h->roll.cfg : nullptr, msg), msg);
    if (plan < 0) return plan;
    if (plan == ENABLE_REPEAT) return out ? imgenv_rollout_outputs(h, out) : IMGENV_OK;  // (with the live n / resets)
    const int want = c->fields;
    const size_t RL = (size_t)h->RL, T = (size_t)c->horizon, F = (size_t)c->final_capacity;
    ObsField fields[OBSF_COUNT];
    handle_obs_fields(h, fields);
    FieldSelection s;
    RTRY(planned(select_feature_fields(FIELDS_ROLLOUT, fields, want, want, s, msg), msg));
    // one zeroed block (launch_plan.h); nothing of the handle changes before it is there
    const RolloutLayout l = plan_rollout_layout(s.row_bytes, s.n, RL, T, F);
    unsigned char* block = nullptr;
    RTRY(feature_block(h, l.total, "imgenv_rollout_enable", &block));
    const imgenv_out& w = h->out;
    imgenv_rollout_out o = {};
    RolloutDev ro;
    memset(&ro, 0, sizeof(ro));
    ro.n_fields = s.n;
    for (int k = 0; k < s.n; k++) {
        const ObsSlot& slot = OBS_SLOTS[s.id[k]];
        const FinalFieldPlan f = plan_final_field(s.row_bytes[k]);
        ro.f[k].ring = block + l.ring[k];
        ro.f[k].fin = block + l.fin[k];
        ro.f[k].src = (const unsigned char*)fields[s.id[k]].src;
        ro.f[k].unit = f.unit;
        ro.f[k].chunks = f.chunks;
        ro.chunks_per_row += f.chunks;
        h->roll.row_bytes[k] = s.row_bytes[k];
        h->roll.field_id[k] = s.id[k];
        obs_slot_put(slot, slot.ring_out, &o, &h->norm.out, ro.f[k].ring);
        obs_slot_put(slot, slot.fin_out, &o, &h->norm.out, ro.f[k].fin);
    }
    // (the working arena, also under IMGENV_FLAG_FULL_REWRITE; IMGENV_ROLLOUT_NORM_REWARDS: what k_norm_apply has just written)
    ro.rew_src = (want & IMGENV_ROLLOUT_NORM_REWARDS) ? h->norm.dev.norm_rewards : w.step_rewards;
    ro.done_src = w.step_dones;
    ro.clean_src = w.step_is_clean;
    ro.info_src = w.step_dones_info;
    o.actions = ro.actions = (float*)(block + l.actions);
    o.rewards = ro.rewards = (float*)(block + l.rewards);
    o.dones = ro.dones = block + l.dones;
    o.is_clean = ro.is_clean = block + l.is_clean;
    o.dones_info = ro.dones_info = (int32_t*)(block + l.dones_info);
    o.final_idx = ro.final_idx = (int32_t*)(block + l.final_idx);
    o.final_slot = ro.final_slot = (int32_t*)(block + l.final_slot);
    o.final_row = ro.final_row = (int32_t*)(block + l.final_row);
    o.final_n = ro.final_n = (uint32_t*)(block + l.final_n);
    ro.F = c->final_capacity;
    o.horizon = c->horizon;
    o.final_capacity = c->final_capacity;
    o.n = -1;
    h->roll.dev = ro;
    h->roll.cfg = *c;
    h->roll.begun = false;
    h->roll.n = 0;
    h->roll.turn = 0;
    return enable_done(h, h->roll, o, out);
}

// the chain's tail (launch_tails), once imgenv_rollout_begin has been called: a step stores transition n and the observation it
// led to in slot n + 1 (rollout_room has refused a step on a full ring), a reset chain moves the rows of slot n it covers into the
// final list and stores the new episode's first observation there
static void tail_rollout(imgenv* h, hipStream_t st, const ChainPlans& k) {
    if (!h->roll.on || !h->roll.begun) return;
    RolloutDev ro = h->roll.dev;
    ro.rows = tail_rows(h, k.is_reset);
    ro.act_src = h->step.actions;
    ro.n = h->roll.n;
    ro.turn = h->roll.turn;
    const LaunchShape g = plan_rollout_launch(h->plan, k.c, ro.chunks_per_row);
    (k.is_reset ? k_rollout<true> : k_rollout<false>)<<<dim3(g.grid), dim3(g.block), 0, st>>>(ro);
    h->launches += 1;
    if (k.is_reset)
        h->roll.turn += 1;
    else
        h->roll.n += 1;
}

extern "C" int imgenv_rollout_outputs(imgenv_t* h, imgenv_rollout_out* out) {
    if (int rc = feature_outputs(h, &imgenv::roll, out, "imgenv_rollout_enable")) return rc;
    out->n = h->roll.begun ? h->roll.n : -1;
    out->resets = (int32_t)h->roll.turn;
    return IMGENV_OK;
}

extern "C" int imgenv_rollout_begin(imgenv_t* h, void* stream) {
    if (!h) FAIL(IMGENV_EINVAL, "null argument");
    RTRY(needs(h->roll.on, "imgenv_rollout_enable"));
    if (!h->step.obs_exists) FAIL(IMGENV_ESTATE, "imgenv_rollout_begin before the first reset: there is no observation yet");
    if (h->step.obs_forked) FAIL(IMGENV_ESTATE, "imgenv_rollout_begin between imgenv_step_begin and imgenv_step_end");
    HIPCHK(hipSetDevice(h->cfg.device));
    hipStream_t st = (hipStream_t)stream;
    const size_t RL = (size_t)h->RL;
    if (!h->roll.begun || h->roll.n > 0) {
        // slot n -> slot 0 (the first time: the live arrays -> slot 0): k_rollout's step instantiation with the scalars off
        RolloutDev ro = h->roll.dev;
        if (h->roll.begun)
            for (int k = 0; k < ro.n_fields; k++) ro.f[k].src = ro.f[k].ring + (size_t)h->roll.n * RL * h->roll.row_bytes[k];
        ro.rewards = nullptr;
        ro.n = -1;
        ro.rows = tail_rows(h, 0);
        const LaunchShape g = plan_rollout_begin_launch(h->plan, ro.chunks_per_row);
        k_rollout<false><<<dim3(g.grid), dim3(g.block), 0, st>>>(ro);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemsetAsync(h->roll.dev.final_idx, 0xFF, ((size_t)h->roll.cfg.horizon + 1) * RL * 4, st));
    HIPCHK(hipMemsetAsync(h->roll.dev.final_n, 0, 8, st));
    h->roll.begun = true;
    h->roll.n = 0;
    h->roll.turn = 0;
    h->step.chain_seq += 1;
    return IMGENV_OK;
}

extern "C" int imgenv_rollout_gae(imgenv_t* h, const float* values, const float* final_values, float gamma, float lam, float* adv, float* ret,
                                  void* stream) {
    if (!h || !values || !adv || !ret) FAIL(IMGENV_EINVAL, "null argument");
    RTRY(needs(h->roll.on, "imgenv_rollout_enable"));
    if (!h->roll.begun) FAIL(IMGENV_ESTATE, "imgenv_rollout_gae before imgenv_rollout_begin");
    if (h->roll.n == 0) return IMGENV_OK;  // (no transition yet: every row of adv / ret is left untouched)
    HIPCHK(hipSetDevice(h->cfg.device));
    const RolloutDev& ro = h->roll.dev;
    const RolloutGaeDev g = {ro.rewards, ro.dones, ro.is_clean, ro.dones_info, ro.final_idx, values, final_values, adv, ret, gamma, lam, h->roll.n, ro.F, h->RL};
    const LaunchShape s = plan_rollout_gae_launch(h->plan);
    k_rollout_gae<<<dim3(s.grid), dim3(s.block), 0, (hipStream_t)stream>>>(g);
    HIPCHK(hipGetLastError());
    return IMGENV_OK;
}

// k_ped_draw's arguments for `n` maps of this handle's geometry drawn from rows of `vec` (ped_draw.h); `out` may come later
static PedDrawDev ped_draw_args(const imgenv* h, const float* vec, const int32_t* rows, uint32_t n, float* out) {
    PedDrawDev d = {};
    d.vec = vec;
    d.rows = rows;
    d.out = out;
    d.n = n;
    d.PV = h->d.PV; d.Hp = h->d.Hp; d.Wp = h->d.Wp;
    d.res = h->d.ped_res; d.inv_res = h->d.ped_inv_res; d.r = h->d.ped_image_r; d.r2 = h->d.ped_image_r2;
    return d;
}
static void launch_ped_draw(PedDrawDev d, hipStream_t st) {
    d.wide = ((size_t)d.Hp * (size_t)d.Wp) % 4 == 0 && ((uintptr_t)d.out & 15) == 0;
    const LaunchShape s = plan_ped_draw_launch(d.n, d.Hp, d.Wp);
    k_ped_draw<<<dim3(s.grid), dim3(s.block), s.lds, st>>>(d);
}

// ---- rollout minibatches (include/imgenv.h; the kernels are csrc/minibatch.h) ----
extern "C" int imgenv_rollout_minibatch_enable(imgenv_t* h, const imgenv_minibatch_cfg* c, imgenv_minibatch_out* out) {
    FeatureMsg msg;
    FeatureFacts facts;
    int want = 0;
    const int plan = planned(minibatch_enable_plan(c, out, feature_facts(h, facts), h ? &h->mb.cfg : nullptr, &want, msg), msg);
    if (plan < 0) return plan;
    if (plan == ENABLE_REPEAT) return out ? imgenv_rollout_minibatch_outputs(h, out) : IMGENV_OK;
    // what the ring keeps, as a catalogue: the buffers' fields come out in the ring's own order
    ObsField ring[OBSF_COUNT] = {};
    for (int k = 0; k < h->roll.dev.n_fields; k++) ring[h->roll.field_id[k]] = {h->roll.dev.f[k].ring, h->roll.row_bytes[k]};
    FieldSelection s;
    RTRY(planned(select_feature_fields(FIELDS_MINIBATCH, ring, want, c->fields, s, msg, ped_maps_row_bytes(facts)), msg));
    // one zeroed block (launch_plan.h); nothing of the handle changes before it is there
    const size_t RL = (size_t)h->RL, T = (size_t)h->roll.cfg.horizon, NB = (size_t)c->buffers;
    const MinibatchLayout l = plan_minibatch_layout(s.row_bytes, s.n, RL, T, (size_t)c->batch, NB);
    unsigned char* block = nullptr;
    RTRY(feature_block(h, l.total, "imgenv_rollout_minibatch_enable", &block));
    MbGatherDev g;
    memset(&g, 0, sizeof(g));
    // the gather's table: the selection without the drawn field (entry `of[k]` of the selection), which is k_ped_draw's
    int of[ROLLOUT_TABLE_FIELDS] = {}, drawn = -1;
    for (int k = 0; k < s.n; k++) {
        if (s.id[k] == OBSF_PED_MAPS_DRAWN) {
            drawn = k;
            continue;
        }
        const FinalFieldPlan f = plan_final_field(s.row_bytes[k]);  // (the ring's own chunking)
        MbGatherField& gf = g.f[g.n_fields];
        gf.ring = (const unsigned char*)ring[s.id[k]].src;
        gf.unit = f.unit;  // (dst: the buffer's, h->mb.dst, at the call)
        gf.chunks = f.chunks;
        g.chunks_per_row += f.chunks;
        of[g.n_fields++] = k;
    }
    if (g.n_fields == 0) g.chunks_per_row = 1;  // (nothing to copy: the one chunk per slot is the scalars' lane)
    imgenv_minibatch_out o = {};
    o.horizon = h->roll.cfg.horizon;
    o.batch = c->batch;
    o.buffers = c->buffers;
    o.fields = want;
    o.valid = (int32_t*)(block + l.valid);
    o.order = (int32_t*)(block + l.order);
    o.valid_n = (uint32_t*)(block + l.valid_n);
    o.norm = (float*)(block + l.norm);
    o.tile_count = (int32_t*)(block + l.tile_count);
    o.tile_base = (int32_t*)(block + l.tile_base);
    o.stat_part = (double*)(block + l.stat_part);
    o.stat_mean = (double*)(block + l.stat_mean);
    for (size_t b = 0; b < NB; b++) {
        imgenv_minibatch_buffer& m = o.buf[b];
        for (int k = 0; k < s.n; k++) obs_slot_put_mb(OBS_SLOTS[s.id[k]], &m, &h->norm.out, (int)b, block + l.field[b][k]);
        for (int k = 0; k < g.n_fields; k++) h->mb.dst[b][k] = block + l.field[b][of[k]];
        if (drawn >= 0) h->mb.draw_dst[b] = (float*)(block + l.field[b][drawn]);
        m.mb_actions = (float*)(block + l.scalar[b][MB_S_ACTIONS]);
        m.mb_rewards = (float*)(block + l.scalar[b][MB_S_REWARDS]);
        m.mb_dones = block + l.scalar[b][MB_S_DONES];
        m.mb_dones_info = (int32_t*)(block + l.scalar[b][MB_S_DONES_INFO]);
        m.mb_index = (int32_t*)(block + l.scalar[b][MB_S_INDEX]);
        m.mb_weight = (float*)(block + l.scalar[b][MB_S_WEIGHT]);
        m.mb_scalars = (float*)(block + l.scalar[b][MB_S_SCALARS]);
    }
    g.order = o.order;
    g.B = (uint32_t)c->batch;
    g.TR = (uint32_t)(T * RL);
    g.actions = h->roll.dev.actions;
    g.rewards = h->roll.dev.rewards;
    g.dones = h->roll.dev.dones;
    g.dones_info = h->roll.dev.dones_info;
    h->mb.draw = {};
    if (drawn >= 0) {
        h->mb.draw = ped_draw_args(h, (const float*)ring[OBS_SLOTS[OBSF_PED_MAPS_DRAWN].from].src, nullptr, g.B, nullptr);
        h->mb.draw.order = o.order;
        h->mb.draw.TR = g.TR;
    }
    h->mb.dev = g;
    h->mb.cfg = *c;
    h->mb.indexed = h->mb.shuffled = false;
    return enable_done(h, h->mb, o, out);
}

extern "C" int imgenv_rollout_minibatch_outputs(imgenv_t* h, imgenv_minibatch_out* out) {
    return feature_outputs(h, &imgenv::mb, out, "imgenv_rollout_minibatch_enable");
}

// the index is of this moment: no chain and no imgenv_rollout_begin since
static int minibatch_fresh(const imgenv* h, const char* who) {
    RTRY(needs(h->mb.on, "imgenv_rollout_minibatch_enable"));
    if (!h->mb.indexed) FAIL(IMGENV_ESTATE, "%s before imgenv_rollout_index", who);
    if (!h->roll.begun || h->mb.gen_n != h->roll.n || h->mb.gen_seq != h->step.chain_seq) FAIL(IMGENV_ESTATE, "%s: rollout changed since imgenv_rollout_index", who);
    return IMGENV_OK;
}

extern "C" int imgenv_rollout_index(imgenv_t* h, void* stream) {
    if (!h) FAIL(IMGENV_EINVAL, "null argument");
    RTRY(needs(h->mb.on, "imgenv_rollout_minibatch_enable"));
    if (!h->roll.begun) FAIL(IMGENV_ESTATE, "imgenv_rollout_index before imgenv_rollout_begin");
    if (h->roll.n == 0) FAIL(IMGENV_ESTATE, "imgenv_rollout_index: no transition is stored yet");
    HIPCHK(hipSetDevice(h->cfg.device));
    hipStream_t st = (hipStream_t)stream;
    const imgenv_minibatch_out& o = h->mb.out;
    const size_t total = (size_t)h->roll.n * (size_t)h->RL;
    const MbIndexDev d = {h->roll.dev.is_clean, o.valid, o.tile_count, o.tile_base, o.valid_n, (uint32_t)total, (uint32_t)plan_mb_tiles(total)};
    const LaunchShape tiles = plan_mb_index_launch(total), one = plan_mb_scan_launch();
    k_mb_count<<<dim3(tiles.grid), dim3(tiles.block), 0, st>>>(d);
    k_mb_scan<<<dim3(one.grid), dim3(one.block), 0, st>>>(d);
    k_mb_scatter<<<dim3(tiles.grid), dim3(tiles.block), 0, st>>>(d);
    HIPCHK(hipGetLastError());
    h->mb.indexed = true;
    h->mb.shuffled = false;
    h->mb.gen_n = h->roll.n;
    h->mb.gen_seq = h->step.chain_seq;
    return IMGENV_OK;
}

extern "C" int imgenv_rollout_stats(imgenv_t* h, const float* x, double eps, float* norm_out, void* stream) {
    if (!h || !x) FAIL(IMGENV_EINVAL, "null argument");
    if (!(eps >= 0.0)) FAIL(IMGENV_EINVAL, "imgenv_rollout_stats: eps %g", eps);
    RTRY(minibatch_fresh(h, "imgenv_rollout_stats"));
    HIPCHK(hipSetDevice(h->cfg.device));
    hipStream_t st = (hipStream_t)stream;
    const imgenv_minibatch_out& o = h->mb.out;
    const size_t total = (size_t)h->mb.gen_n * (size_t)h->RL;
    const MbStatsDev s = {x, o.valid, o.valid_n, o.stat_part, o.stat_mean, norm_out ? norm_out : o.norm, eps, (uint32_t)plan_mb_stats_tiles(total)};
    const LaunchShape tiles = plan_mb_stats_launch(total), one = plan_mb_stats_final_launch();
    k_mb_stats<false><<<dim3(tiles.grid), dim3(tiles.block), 0, st>>>(s);
    k_mb_stats_final<false><<<dim3(one.grid), dim3(one.block), 0, st>>>(s);
    k_mb_stats<true><<<dim3(tiles.grid), dim3(tiles.block), 0, st>>>(s);
    k_mb_stats_final<true><<<dim3(one.grid), dim3(one.block), 0, st>>>(s);
    HIPCHK(hipGetLastError());
    return IMGENV_OK;
}

extern "C" int imgenv_rollout_shuffle(imgenv_t* h, uint32_t seed_lo, uint32_t seed_hi, void* stream) {
    if (!h) FAIL(IMGENV_EINVAL, "null argument");
    RTRY(minibatch_fresh(h, "imgenv_rollout_shuffle"));
    HIPCHK(hipSetDevice(h->cfg.device));
    const imgenv_minibatch_out& o = h->mb.out;
    const MbShuffleDev s = {o.valid, o.valid_n, o.order, h->mb.dev.TR, mb_keys(seed_lo, seed_hi)};
    const LaunchShape g = plan_mb_shuffle_launch(s.TR);
    k_mb_shuffle<<<dim3(g.grid), dim3(g.block), 0, (hipStream_t)stream>>>(s);
    HIPCHK(hipGetLastError());
    h->mb.shuffled = true;
    return IMGENV_OK;
}

extern "C" int imgenv_rollout_minibatch(imgenv_t* h, const imgenv_minibatch_args* a, void* stream) {
    if (!a) FAIL(IMGENV_EINVAL, "null argument");
    if (a->struct_size != (int32_t)sizeof(imgenv_minibatch_args))
        FAIL(IMGENV_EINVAL, "imgenv_minibatch_args.struct_size %d (this library's is %d)", a->struct_size, (int)sizeof(imgenv_minibatch_args));
    if (a->j < 0) FAIL(IMGENV_EINVAL, "imgenv_minibatch_args.j %d", a->j);
    if (a->n_scalars < 0 || a->n_scalars > IMGENV_MB_MAX_SCALARS) FAIL(IMGENV_EINVAL, "imgenv_minibatch_args.n_scalars %d: 0 .. %d", a->n_scalars, IMGENV_MB_MAX_SCALARS);
    if (a->normalise < -1 || a->normalise >= a->n_scalars) FAIL(IMGENV_EINVAL, "imgenv_minibatch_args.normalise %d: -1 or an index below n_scalars %d", a->normalise, a->n_scalars);
    for (int s = 0; s < a->n_scalars; s++)
        if (!a->scalars[s]) FAIL(IMGENV_EINVAL, "imgenv_minibatch_args.scalars[%d] is null", s);
    if (!h) FAIL(IMGENV_EINVAL, "null argument");
    RTRY(needs(h->mb.on, "imgenv_rollout_minibatch_enable"));
    if (a->buffer < 0 || a->buffer >= h->mb.cfg.buffers) FAIL(IMGENV_EINVAL, "imgenv_minibatch_args.buffer %d: 0 .. %d", a->buffer, h->mb.cfg.buffers - 1);
    RTRY(minibatch_fresh(h, "imgenv_rollout_minibatch"));
    if (!h->mb.shuffled) FAIL(IMGENV_ESTATE, "imgenv_rollout_minibatch before imgenv_rollout_shuffle");
    HIPCHK(hipSetDevice(h->cfg.device));
    const imgenv_minibatch_buffer& m = h->mb.out.buf[a->buffer];
    MbGatherDev g = h->mb.dev;
    for (int k = 0; k < g.n_fields; k++) g.f[k].dst = h->mb.dst[a->buffer][k];
    g.first = (size_t)a->j * (size_t)g.B;
    g.mb_actions = m.mb_actions;
    g.mb_rewards = m.mb_rewards;
    g.mb_dones = m.mb_dones;
    g.mb_dones_info = m.mb_dones_info;
    g.mb_index = m.mb_index;
    g.mb_weight = m.mb_weight;
    g.mb_scalars = m.mb_scalars;
    for (int s = 0; s < a->n_scalars; s++) g.scalars[s] = a->scalars[s];
    g.n_scalars = a->n_scalars;
    g.normalise = a->normalise;
    g.norm = a->norm ? a->norm : h->mb.out.norm;
    const LaunchShape s = plan_mb_gather_launch(g.B, g.chunks_per_row);
    k_rollout_gather<<<dim3(s.grid), dim3(s.block), 0, (hipStream_t)stream>>>(g);
    if (h->mb.draw.vec) {  // IMGENV_ROLLOUT_PED_MAPS_DRAWN: mb_ped_maps of the same slots, one more launch
        PedDrawDev d = h->mb.draw;
        d.out = h->mb.draw_dst[a->buffer];
        d.first = g.first;
        launch_ped_draw(d, (hipStream_t)stream);
    }
    HIPCHK(hipGetLastError());
    return IMGENV_OK;
}


// ---- sequence minibatches (include/imgenv.h; the kernels are csrc/sequences.h) ----
extern "C" int imgenv_rollout_seq_enable(imgenv_t* h, const imgenv_seq_cfg* c, imgenv_seq_out* out) {
    FeatureMsg msg;
    FeatureFacts facts;
    int want = 0;
    const int plan = planned(seq_enable_plan(c, out, feature_facts(h, facts), h ? &h->seq.cfg : nullptr, &want, msg), msg);
    if (plan < 0) return plan;
    if (plan == ENABLE_REPEAT) return out ? imgenv_rollout_seq_outputs(h, out) : IMGENV_OK;
    // what the ring keeps, as a catalogue: the buffers' fields come out in the ring's own order
    ObsField ring[OBSF_COUNT] = {};
    for (int k = 0; k < h->roll.dev.n_fields; k++) ring[h->roll.field_id[k]] = {h->roll.dev.f[k].ring, h->roll.row_bytes[k]};
    FieldSelection s;
    RTRY(planned(select_feature_fields(FIELDS_SEQ, ring, want, c->fields, s, msg, ped_maps_row_bytes(facts)), msg));
    // one zeroed block (launch_plan.h); nothing of the handle changes before it is there
    const size_t RL = (size_t)h->RL, T = (size_t)h->roll.cfg.horizon, NB = (size_t)c->buffers, L = (size_t)c->length, Bs = (size_t)c->batch;
    const size_t state_bytes[SEQ_MAX_STATES] = {(size_t)c->state_bytes[0], (size_t)c->state_bytes[1]};
    const SeqLayout l = plan_seq_layout(s.row_bytes, s.n, RL, T, L, Bs, NB, state_bytes);
    unsigned char* block = nullptr;
    RTRY(feature_block(h, l.total, "imgenv_rollout_seq_enable", &block));
    SeqGatherDev g;
    memset(&g, 0, sizeof(g));
    // the gather's table: the selection without the drawn field (entry `of[k]` of the selection), which is k_ped_draw's
    int of[ROLLOUT_TABLE_FIELDS] = {}, drawn = -1;
    for (int k = 0; k < s.n; k++) {
        if (s.id[k] == OBSF_PED_MAPS_DRAWN) {
            drawn = k;
            continue;
        }
        const FinalFieldPlan f = plan_final_field(s.row_bytes[k]);  // (the ring's own chunking)
        MbGatherField& gf = g.f[g.n_fields];
        gf.ring = (const unsigned char*)ring[s.id[k]].src;
        gf.unit = f.unit;  // (dst: the buffer's, h->seq.dst, at the call)
        gf.chunks = f.chunks;
        g.chunks_per_row += f.chunks;
        of[g.n_fields++] = k;
    }
    if (g.n_fields == 0) g.chunks_per_row = 1;  // (nothing to copy: the one chunk per step is the scalars' lane)
    for (int a = 0; a < SEQ_MAX_STATES; a++) {
        const FinalFieldPlan f = plan_final_field(state_bytes[a]);
        g.st[a].unit = f.unit;
        g.st[a].chunks = state_bytes[a] ? f.chunks : 0;
        g.state_chunks += g.st[a].chunks;
    }
    imgenv_seq_out o = {};
    o.horizon = h->roll.cfg.horizon;
    o.length = c->length;
    o.batch = c->batch;
    o.buffers = c->buffers;
    o.fields = want;
    o.max_sequences = (int32_t)(plan_seq_chunks(T, L) * RL);
    o.state_bytes[0] = c->state_bytes[0];
    o.state_bytes[1] = c->state_bytes[1];
    o.seq_flag = block + l.flag;
    o.seq_valid = (int32_t*)(block + l.valid);
    o.seq_order = (int32_t*)(block + l.order);
    o.seq_valid_n = (uint32_t*)(block + l.valid_n);
    o.tile_count = (int32_t*)(block + l.tile_count);
    o.tile_base = (int32_t*)(block + l.tile_base);
    for (size_t b = 0; b < NB; b++) {
        imgenv_seq_buffer& m = o.buf[b];
        for (int k = 0; k < s.n; k++) obs_slot_put_seq(OBS_SLOTS[s.id[k]], &m, block + l.field[b][k]);
        for (int k = 0; k < g.n_fields; k++) h->seq.dst[b][k] = block + l.field[b][of[k]];
        if (drawn >= 0) h->seq.draw_dst[b] = (float*)(block + l.field[b][drawn]);
        m.mb_actions = (float*)(block + l.scalar[b][SEQ_S_ACTIONS]);
        m.mb_rewards = (float*)(block + l.scalar[b][SEQ_S_REWARDS]);
        m.mb_dones = block + l.scalar[b][SEQ_S_DONES];
        m.mb_dones_info = (int32_t*)(block + l.scalar[b][SEQ_S_DONES_INFO]);
        m.mb_index = (int32_t*)(block + l.scalar[b][SEQ_S_INDEX]);
        m.mb_weight = (float*)(block + l.scalar[b][SEQ_S_WEIGHT]);
        m.mb_first = block + l.scalar[b][SEQ_S_FIRST];
        m.mb_scalars = (float*)(block + l.scalar[b][SEQ_S_SCALARS]);
        m.mb_seq = (int32_t*)(block + l.scalar[b][SEQ_S_SEQ]);
        m.mb_seq_len = (int32_t*)(block + l.scalar[b][SEQ_S_SEQ_LEN]);
        for (int a = 0; a < SEQ_MAX_STATES; a++) m.mb_seq_state[a] = state_bytes[a] ? block + l.scalar[b][SEQ_S_STATE0 + a] : nullptr;
    }
    g.order = o.seq_order;
    g.Bs = (uint32_t)c->batch;
    g.L = (uint32_t)c->length;
    g.R = (uint32_t)RL;
    g.S = (uint32_t)o.max_sequences;
    g.actions = h->roll.dev.actions;
    g.rewards = h->roll.dev.rewards;
    g.dones = h->roll.dev.dones;
    g.is_clean = h->roll.dev.is_clean;
    g.dones_info = h->roll.dev.dones_info;
    g.final_idx = h->roll.dev.final_idx;
    h->seq.draw = {};
    if (drawn >= 0) h->seq.draw = ped_draw_args(h, (const float*)ring[OBS_SLOTS[OBSF_PED_MAPS_DRAWN].from].src, nullptr, (uint32_t)(L * Bs), nullptr);
    h->seq.dev = g;
    h->seq.cfg = *c;
    h->seq.indexed = h->seq.shuffled = false;
    return enable_done(h, h->seq, o, out);
}

extern "C" int imgenv_rollout_seq_outputs(imgenv_t* h, imgenv_seq_out* out) {
    return feature_outputs(h, &imgenv::seq, out, "imgenv_rollout_seq_enable");
}

// the index is of this moment: no chain and no imgenv_rollout_begin since
static int seq_fresh(const imgenv* h, const char* who) {
    RTRY(needs(h->seq.on, "imgenv_rollout_seq_enable"));
    if (!h->seq.indexed) FAIL(IMGENV_ESTATE, "%s before imgenv_rollout_seq_index", who);
    if (!h->roll.begun || h->seq.gen_n != h->roll.n || h->seq.gen_seq != h->step.chain_seq) FAIL(IMGENV_ESTATE, "%s: rollout changed since imgenv_rollout_seq_index", who);
    return IMGENV_OK;
}

extern "C" int imgenv_rollout_seq_index(imgenv_t* h, void* stream) {
    if (!h) FAIL(IMGENV_EINVAL, "null argument");
    RTRY(needs(h->seq.on, "imgenv_rollout_seq_enable"));
    if (!h->roll.begun) FAIL(IMGENV_ESTATE, "imgenv_rollout_seq_index before imgenv_rollout_begin");
    if (h->roll.n == 0) FAIL(IMGENV_ESTATE, "imgenv_rollout_seq_index: no transition is stored yet");
    HIPCHK(hipSetDevice(h->cfg.device));
    hipStream_t st = (hipStream_t)stream;
    const imgenv_seq_out& o = h->seq.out;
    const SeqGatherDev& g = h->seq.dev;
    const size_t total = plan_seq_chunks((size_t)h->roll.n, (size_t)g.L) * (size_t)g.R;  // C R <= C_max R
    const SeqFlagDev f = {h->roll.dev.is_clean, o.seq_flag, g.R, g.L, (uint32_t)h->roll.n, (uint32_t)total};
    const MbIndexDev d = {o.seq_flag, o.seq_valid, o.tile_count, o.tile_base, o.seq_valid_n, (uint32_t)total, (uint32_t)plan_mb_tiles(total)};
    const LaunchShape lanes = plan_seq_flag_launch(total), tiles = plan_mb_index_launch(total), one = plan_mb_scan_launch();
    k_seq_flag<<<dim3(lanes.grid), dim3(lanes.block), 0, st>>>(f);
    k_mb_count<<<dim3(tiles.grid), dim3(tiles.block), 0, st>>>(d);
    k_mb_scan<<<dim3(one.grid), dim3(one.block), 0, st>>>(d);
    k_mb_scatter<<<dim3(tiles.grid), dim3(tiles.block), 0, st>>>(d);
    HIPCHK(hipGetLastError());
    h->seq.indexed = true;
    h->seq.shuffled = false;
    h->seq.gen_n = h->roll.n;
    h->seq.gen_seq = h->step.chain_seq;
    return IMGENV_OK;
}

extern "C" int imgenv_rollout_seq_shuffle(imgenv_t* h, uint32_t seed_lo, uint32_t seed_hi, void* stream) {
    if (!h) FAIL(IMGENV_EINVAL, "null argument");
    RTRY(seq_fresh(h, "imgenv_rollout_seq_shuffle"));
    HIPCHK(hipSetDevice(h->cfg.device));
    const imgenv_seq_out& o = h->seq.out;
    const MbShuffleDev s = {o.seq_valid, o.seq_valid_n, o.seq_order, h->seq.dev.S, mb_keys(seed_lo, seed_hi)};
    const LaunchShape g = plan_mb_shuffle_launch(s.TR);
    k_mb_shuffle<<<dim3(g.grid), dim3(g.block), 0, (hipStream_t)stream>>>(s);
    HIPCHK(hipGetLastError());
    h->seq.shuffled = true;
    return IMGENV_OK;
}

extern "C" int imgenv_rollout_seq_minibatch(imgenv_t* h, const imgenv_seq_args* a, void* stream) {
    if (!a) FAIL(IMGENV_EINVAL, "null argument");
    if (a->struct_size != (int32_t)sizeof(imgenv_seq_args))
        FAIL(IMGENV_EINVAL, "imgenv_seq_args.struct_size %d (this library's is %d)", a->struct_size, (int)sizeof(imgenv_seq_args));
    if (a->j < 0) FAIL(IMGENV_EINVAL, "imgenv_seq_args.j %d", a->j);
    if (a->n_scalars < 0 || a->n_scalars > IMGENV_MB_MAX_SCALARS) FAIL(IMGENV_EINVAL, "imgenv_seq_args.n_scalars %d: 0 .. %d", a->n_scalars, IMGENV_MB_MAX_SCALARS);
    if (a->normalise < -1 || a->normalise >= a->n_scalars) FAIL(IMGENV_EINVAL, "imgenv_seq_args.normalise %d: -1 or an index below n_scalars %d", a->normalise, a->n_scalars);
    for (int s = 0; s < a->n_scalars; s++)
        if (!a->scalars[s]) FAIL(IMGENV_EINVAL, "imgenv_seq_args.scalars[%d] is null", s);
    if (a->normalise >= 0 && !a->norm) FAIL(IMGENV_EINVAL, "imgenv_seq_args.norm is null with normalise %d", a->normalise);
    if (!h) FAIL(IMGENV_EINVAL, "null argument");
    RTRY(needs(h->seq.on, "imgenv_rollout_seq_enable"));
    if (a->buffer < 0 || a->buffer >= h->seq.cfg.buffers) FAIL(IMGENV_EINVAL, "imgenv_seq_args.buffer %d: 0 .. %d", a->buffer, h->seq.cfg.buffers - 1);
    for (int q = 0; q < SEQ_MAX_STATES; q++)
        if (h->seq.cfg.state_bytes[q] > 0 && (!a->states[q] || ((uintptr_t)a->states[q] & 15)))
            FAIL(IMGENV_EINVAL, "imgenv_seq_args.states[%d] is %s", q, a->states[q] ? "not 16-byte aligned" : "null");
    RTRY(seq_fresh(h, "imgenv_rollout_seq_minibatch"));
    if (!h->seq.shuffled) FAIL(IMGENV_ESTATE, "imgenv_rollout_seq_minibatch before imgenv_rollout_seq_shuffle");
    HIPCHK(hipSetDevice(h->cfg.device));
    const imgenv_seq_buffer& m = h->seq.out.buf[a->buffer];
    SeqGatherDev g = h->seq.dev;
    for (int k = 0; k < g.n_fields; k++) g.f[k].dst = h->seq.dst[a->buffer][k];
    for (int q = 0; q < SEQ_MAX_STATES; q++) {
        g.st[q].src = (const unsigned char*)a->states[q];
        g.st[q].dst = m.mb_seq_state[q];
    }
    g.first = (size_t)a->j * (size_t)g.Bs;
    g.n = h->seq.gen_n;
    g.mb_actions = m.mb_actions;
    g.mb_rewards = m.mb_rewards;
    g.mb_dones = m.mb_dones;
    g.mb_dones_info = m.mb_dones_info;
    g.mb_index = m.mb_index;
    g.mb_weight = m.mb_weight;
    g.mb_first = m.mb_first;
    g.mb_scalars = m.mb_scalars;
    g.mb_seq = m.mb_seq;
    g.mb_seq_len = m.mb_seq_len;
    for (int s = 0; s < a->n_scalars; s++) g.scalars[s] = a->scalars[s];
    g.n_scalars = a->n_scalars;
    g.normalise = a->normalise;
    g.norm = a->norm;
    const LaunchShape s = plan_seq_gather_launch(g.L, g.Bs, g.chunks_per_row, g.state_chunks);
    k_rollout_seq_gather<<<dim3(s.grid), dim3(s.block), 0, (hipStream_t)stream>>>(g);
    if (h->seq.draw.vec) {  // IMGENV_ROLLOUT_PED_MAPS_DRAWN: mb_ped_maps of the same steps, one more launch, the buffer's mb_index its rows
        PedDrawDev d = h->seq.draw;
        d.out = h->seq.draw_dst[a->buffer];
        d.rows = m.mb_index;
        launch_ped_draw(d, (hipStream_t)stream);
    }
    HIPCHK(hipGetLastError());
    return IMGENV_OK;
}

// ---- pedestrian maps drawn from pedestrian vectors (include/imgenv.h; the kernel is csrc/ped_draw.h) ----
extern "C" int imgenv_ped_maps_draw(imgenv_t* h, const float* ped_vectors, const int32_t* rows, int64_t n, float* out, void* stream) {
    if (!h || !ped_vectors || !out) FAIL(IMGENV_EINVAL, "null argument");
    if (n < 0 || n > 0x7fffffff) FAIL(IMGENV_EINVAL, "imgenv_ped_maps_draw: n %lld", (long long)n);
    if (h->P <= 0 || h->out.ped_vec_len <= 0) FAIL(IMGENV_EINVAL, "imgenv_ped_maps_draw on a handle without pedestrians");
    if (!plan_ped_draw_fits(h->d.Hp, h->d.Wp))
        FAIL(IMGENV_EINVAL, "imgenv_ped_maps_draw: pedestrian maps of %d x %d cells (a plane of %d bytes at most)", h->d.Hp, h->d.Wp, PED_DRAW_LDS_BYTES);
    if (n == 0) return IMGENV_OK;
    HIPCHK(hipSetDevice(h->cfg.device));
    launch_ped_draw(ped_draw_args(h, ped_vectors, rows, (uint32_t)n, out), (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return IMGENV_OK;
}

extern "C" int imgenv_cv_resize_u8(int kind, const uint8_t* src, int32_t sh, int32_t sw, uint8_t* dst, int32_t dh, int32_t dw) {
    if (!src || !dst || sh < 1 || sw < 1 || dh < 1 || dw < 1 || (kind != 0 && kind != 1)) FAIL(IMGENV_EINVAL, "bad argument");
    cv_resize_u8(kind == 1, src, sh, sw, dst, dh, dw);
    return IMGENV_OK;
}

extern "C" int imgenv_step_launches(imgenv_t* h) { return h ? h->launches : 0; }
extern "C" int imgenv_layer_mode(imgenv_t* h) {
    if (!h) return -1;
    return h->plan.layer | (h->d.sum_shard ? 4 : 0) | (h->early && h->gates_work ? 8 : 0) | (h->crowd.can ? 16 : 0);
}

// debug: read (and clear) the per-phase cycle counters of IMGENV_PHASE_PROFILE builds
extern "C" int imgenv_debug_phases(imgenv_t* h, unsigned long long* out16) {
    if (!h || !out16) FAIL(IMGENV_EINVAL, "null argument");
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out16, h->d.prof, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    HIPCHK(hipMemset(h->d.prof, 0, 16 * sizeof(unsigned long long)));
    return IMGENV_OK;
}
// debug: the 32 free-form marks of profile builds
extern "C" int imgenv_debug_marks(imgenv_t* h, unsigned long long* out32) {
    if (!h || !out32) FAIL(IMGENV_EINVAL, "null argument");
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out32, h->d.dbg, 32 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return IMGENV_OK;
}
// debug / tests: the quadtree of world `world`'s social-force crowd as a digest that does not depend on how the nodes are numbered --
// node count, member entries, a sum of per-leaf hashes (rectangle + sorted members), a sum of per-agent hashes (the rectangle the
// agent's treehash entry points at).  tests/test_gpu_parity.py holds it to the oracle's tree (oracle_sfm.c: sfm_tree_digest) step by step.
extern "C" int imgenv_debug_sfm_tree(imgenv_t* h, int32_t world, uint64_t* out8 /* [8]: node count, member entries, leaf-hash sum, agent-hash sum, 256 membership bits */) {
    if (!h || !out8) FAIL(IMGENV_EINVAL, "null argument");
    const SfmDev& f = h->d.sfm;
    if (h->cfg.ped_scene_type != IMGENV_SCENE_PEDSIM || f.n <= 0 || world < 0 || world >= f.W) FAIL(IMGENV_EINVAL, "no social-force crowd %d", world);
    HIPCHK(hipDeviceSynchronize());
    int n_nodes = 0;
    HIPCHK(hipMemcpy(&n_nodes, f.n_nodes + world, sizeof(int), hipMemcpyDeviceToHost));
    if (n_nodes < 1 || n_nodes > f.cap_nodes) FAIL(IMGENV_EDEVICE, "quadtree node count %d", n_nodes);
    std::vector<SfmNode> nodes((size_t)n_nodes);
    std::vector<int> hash((size_t)f.n);
    HIPCHK(hipMemcpy(nodes.data(), f.nodes + (size_t)world * f.cap_nodes, sizeof(SfmNode) * (size_t)n_nodes, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hash.data(), f.treehash + (size_t)world * f.n, sizeof(int) * (size_t)f.n, hipMemcpyDeviceToHost));
    auto mix = [](uint64_t a, uint64_t v) { return (a ^ v) * 0x100000001b3ull; };
    auto bits = [](double v) {
        uint64_t b;
        memcpy(&b, &v, sizeof(b));
        return b;
    };
    auto rect = [&](uint64_t a, const SfmNode& q) { return mix(mix(mix(mix(a, bits(q.x)), bits(q.y)), bits(q.w)), bits(q.h)); };
    uint64_t members = 0, leaves = 0, agents = 0;
    out8[4] = out8[5] = out8[6] = out8[7] = 0;  // one bit per agent that is a member of some leaf
    for (const SfmNode& q : nodes) {
        if (!q.isleaf || q.n_agents == 0) continue;
        uint64_t a = mix(rect(0xcbf29ce484222325ull, q), (uint64_t)q.n_agents);
        for (int e = 0; e < q.n_agents; e++) {
            a = mix(a, (uint64_t)q.agents[e]);
            if (q.agents[e] >= 0 && q.agents[e] < 256) out8[4 + (q.agents[e] >> 6)] |= 1ull << (q.agents[e] & 63);
        }
        leaves += a;
        members += (uint64_t)q.n_agents;
    }
    for (int a = 0; a < f.n; a++) {
        if (hash[a] < 0 || hash[a] >= n_nodes) FAIL(IMGENV_EDEVICE, "treehash[%d] = %d", a, hash[a]);
        agents += rect(mix(0xcbf29ce484222325ull, (uint64_t)a), nodes[(size_t)hash[a]]);
    }
    out8[0] = (uint64_t)n_nodes; out8[1] = members; out8[2] = leaves; out8[3] = agents;
    return IMGENV_OK;
}
// debug: per-wave (start, end, hw id, 0) records of the last k_view [0, 4 RL) and k_obs [4 RL, 8 RL) launches
extern "C" int imgenv_debug_waves(imgenv_t* h, unsigned long long* out) {
    if (!h || !out) FAIL(IMGENV_EINVAL, "null argument");
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, h->d.prof + 16, 12 * (size_t)h->RL * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return IMGENV_OK;
}
