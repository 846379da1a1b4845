// Which kernel instantiations a handle runs, on the CPU: the committed headers (csrc/create_plan.h, csrc/launch_plan.h) asked the way
// imgenv_hip.hip asks them.  tests/test_variant_census.py builds and runs this (tests/variant_matrix.py writes its input).
//
//   variant_census            reads one case per line on stdin (key=value words, see parse_case) and prints, per chain of launches the
//                             case runs -- the reset, a plain step, a reset of `listed` worlds -- one line
//                                 <name> <chain> <word> <word> ...
//                             whose words are the instantiations (k_view<pow2,a4,stamp,nw>, k_raster<pow2,layer,nw>, ...) and the chain's
//                             flags (fuse_move=1, early_step=0, split=1, ...).  A step is printed once per outcome of the one fact
//                             that exists only on a live handle, gates_work (chains step/gates=0 and step/gates=1).
//   variant_census --lattice  walks a lattice of handle facts around every threshold of the plan and prints every word it meets, once.
//
// No rule of the plan is written here: every decision below is a call into the headers.  What IS mirrored from imgenv_hip.hip is
// plumbing -- plan_facts (CreatePlan -> PlanHandle), chain_facts / set_active (what a chain covers), create_classes (one class per
// distinct shape, size and sensor), and the order in which a chain asks for its plans (imgenv_step_begin, launch_views).  The GPU
// matrix (tests/test_gpu_variant_matrix.py) holds that mirror to the library: it asserts the launch counts per kernel id that these
// lines imply.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <map>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#define WAVE_SZ 64  // (host_tables.h: the .hip defines it in front of its includes)
#include "../../img_env_amd/csrc/create_plan.h"

static std::string fmt(const char* f, ...) {
    char b[256];
    va_list ap;
    va_start(ap, f);
    vsnprintf(b, sizeof(b), f, ap);
    va_end(ap);
    return b;
}
static const char* const LAYERS[3] = {"COMPOSED", "STAMP", "SUM"};
typedef std::vector<std::string> Words;

// ---------------------------------------------------------------------------------------- a chain's words
static void raster_words(const PlanHandle& h, const PlanChain& c, Words& o) {  // launch_rasters
    if (const RasterPackPlan k = plan_raster_pack(h, c); k.rpw) {
        o.push_back(fmt("k_raster_pack<%d,%d>", (int)h.pow2, k.rpw));
        return;
    }
    const RasterPlan r = plan_rasters(h, c);
    o.push_back(fmt("%s<%d,%s,%d>", r.move ? "k_move_raster" : "k_raster", (int)h.pow2, LAYERS[h.layer], r.nw));
    o.push_back(fmt("split=%d", r.split != 0));
    o.push_back(fmt("roomy=%d", (int)r.roomy));
}
static void view_words(const PlanHandle& h, const PlanChain& c, Words& o) {  // launch_compose_views
    const ViewPlan v = plan_views(h, c);
    if (h.layer == LAYER_COMPOSED) o.push_back("k_compose");
    if (!h.big_view) {
        o.push_back(fmt("k_view<%d,%d,%d,%d>", (int)h.pow2, (int)h.view_a4, (int)(h.layer == LAYER_STAMP), v.nw));
        o.push_back(fmt("lds_bound=%d", (int)v.lds_bound));
        return;
    }
    o.push_back(fmt("k_crop_big<%d>", v.crop_sel));
    o.push_back(fmt("k_beams_big<%d,%d,%d>", (int)h.pow2, (int)(h.layer == LAYER_STAMP), (int)h.big_bits_in_lds));
    if (v.taps) o.push_back("k_taps_big");
    if (v.full) o.push_back("k_fullview_big");
}
static void obs_words(const PlanHandle& h, Words& o) {
    if (h.P > 0) o.push_back(fmt("k_obs<%d>", h.obs_E));
}
// what a chain covers (set_active): every world, or `n` listed ones
static PlanChain chain_over(const PlanHandle& h, int n_listed) {
    PlanChain c;
    if (n_listed <= 0) {
        c.act_nw = h.W; c.act_nl = h.RL; c.act_ng = h.R; c.act_np = h.P;
    } else {
        c.listed = true;
        c.act_nw = n_listed; c.act_nl = c.act_ng = n_listed * h.Rw; c.act_np = n_listed * h.Pw;
    }
    c.act_cells = (size_t)c.act_nw * h.Gs;
    return c;
}
// imgenv_reset / imgenv_reset_worlds: launch_views(is_reset)
static Words reset_chain(const PlanHandle& h, int n_listed) {
    Words o;
    PlanChain c = chain_over(h, n_listed);
    c.is_reset = true;
    const SidePlan s = plan_side(h, c);
    if (s.remote_only) o.push_back(fmt("k_remote<%d>", (int)h.pow2));
    else raster_words(h, c, o);
    obs_words(h, o);
    view_words(h, c, o);
    return o;
}
// imgenv_step (a handle that owns its world) or imgenv_step_begin + imgenv_step_end around the caller's exchange (a shard), in the
// steady state: a solve and a view have run, no chain is open
static Words step_chain(PlanHandle h, bool gates_work, bool sfm_ahead, bool early_off, bool split_step = false) {
    Words o;
    h.gates_work = gates_work;
    PlanChain c = chain_over(h, 0);
    c.in_step = !h.sharded && !split_step;
    c.orca_ran = c.view_ran = true;
    c.crowd_ahead = sfm_ahead;
    c.early_off = early_off;
    c.stamp_seq = 1;
    const StepPlan sp = plan_step(h, c);
    o.push_back(fmt("fuse_move=%d", (int)sp.fuse_move));
    o.push_back(fmt("early_step=%d", (int)sp.early_step));
    o.push_back(fmt("serial_move=%d", (int)sp.serial_move));
    PlanChain cr = c;
    if (sp.sum_shard_now) {
        cr.moved = cr.local_only = true;
        raster_words(h, cr, o);
    } else if (sp.fuse_move) {
        cr.moved = true;
        raster_words(h, cr, o);
    } else {
        o.push_back(sp.serial_move ? "k_integrate_serial" : "k_integrate");
        cr.local_only = h.sum_shard;  // (a SUM shard draws its own robots in front of the exchange)
        raster_words(h, cr, o);
    }
    const SidePlan s = plan_side(h, c);
    if (s.remote_only) o.push_back(fmt("k_remote<%d>", (int)h.pow2));
    obs_words(h, o);
    view_words(h, c, o);
    return o;
}

// ---------------------------------------------------------------------------------------- cases: from a configuration
struct Case {
    std::string name;
    imgenv_cfg cfg;
    int Hg = 0, Wg = 0, listed = 0, pack = -1;
    bool early_off = false, serial = false, split_step = false;
    std::vector<std::vector<float>> rc, pc;  // distinct classes: shape, size[4], sensor[2] / shape, size[6]
};
static std::vector<float> floats(const std::string& s) {
    std::vector<float> v;
    std::stringstream ss(s);
    std::string w;
    while (std::getline(ss, w, ':')) v.push_back(strtof(w.c_str(), nullptr));
    return v;
}
static bool parse_case(const std::string& line, Case& k) {
    memset(&k.cfg, 0, sizeof(k.cfg));
    imgenv_cfg& c = k.cfg;
    c.abi_version = IMGENV_ABI_VERSION;
    c.struct_size = (int32_t)sizeof(imgenv_cfg);
    c.state_dim = 3;
    c.ped_vec_dim = 7;
    c.ped_image_size[0] = c.ped_image_size[1] = 48;
    c.n_worlds = 1;
    std::stringstream ss(line);
    std::string w;
    while (ss >> w) {
        const size_t eq = w.find('=');
        if (eq == std::string::npos) return false;
        const std::string key = w.substr(0, eq), val = w.substr(eq + 1);
        const double d = strtod(val.c_str(), nullptr);
        if (key == "name") k.name = val;
        else if (key == "n_robots") c.n_robots = (int)d;
        else if (key == "robot_begin") c.robot_begin = (int)d;
        else if (key == "robot_end") c.robot_end = (int)d;
        else if (key == "n_peds") c.n_peds = (int)d;
        else if (key == "n_worlds") c.n_worlds = (int)d;
        else if (key == "max_ped") c.max_ped = (int)d;
        else if (key == "view_resolution") c.view_resolution = (float)d;
        else if (key == "global_resolution") c.global_resolution = (float)d;
        else if (key == "view_width") c.view_width = (float)d;
        else if (key == "view_height") c.view_height = (float)d;
        else if (key == "view_angle_begin") c.view_angle_begin = (float)d;
        else if (key == "view_angle_end") c.view_angle_end = (float)d;
        else if (key == "view_min_dist") c.view_min_dist = (float)d;
        else if (key == "view_max_dist") c.view_max_dist = (float)d;
        else if (key == "step_hz") c.step_hz = (float)d;
        else if (key == "state_dim") c.state_dim = (int)d;
        else if (key == "use_laser") c.use_laser = (int)d;
        else if (key == "range_total") c.range_total = (int)d;
        else if (key == "ped_scene_type") c.ped_scene_type = (int)d;
        else if (key == "relation_ped_robo") c.relation_ped_robo = (int)d;
        else if (key == "beep_r") c.beep_r = (float)d;
        else if (key == "ped_ca_p") c.ped_ca_p = (float)d;
        else if (key == "flags") c.flags = (uint32_t)d;
        else if (key == "image_w") c.image_size[0] = (int)d;
        else if (key == "image_h") c.image_size[1] = (int)d;
        else if (key == "Hg") k.Hg = (int)d;
        else if (key == "Wg") k.Wg = (int)d;
        else if (key == "listed") k.listed = (int)d;
        else if (key == "raster_pack") k.pack = (int)d;   // IMGENV_RASTER_PACK as the handle's creation finds it (-1: unset)
        else if (key == "early_obs_off") k.early_off = d != 0;  // IMGENV_EARLY_OBS=0
        else if (key == "serial") k.serial = d != 0;            // IMGENV_SERIAL=1
        else if (key == "split_step") k.split_step = d != 0;    // a handle that owns its world stepped through imgenv_step_begin / _end
        else if (key == "rc") k.rc.push_back(floats(val));
        else if (key == "pc") k.pc.push_back(floats(val));
        else return false;
    }
    for (const auto& r : k.rc)
        if (r.size() != 7) return false;
    for (const auto& p : k.pc)
        if (p.size() != 7) return false;
    return !k.name.empty() && !k.rc.empty() && (c.n_peds == 0 || !k.pc.empty());
}

static int run_case(const Case& k) {
    const imgenv_cfg& c = k.cfg;
    CreateMsg msg;
    CreateArgs a;
    int Hg = k.Hg, Wg = k.Wg;
    if (create_check_args(&c, true, true, Hg, Wg, a, msg) || create_grid_size(c, a.W, Hg, Wg, msg)) {
        printf("%s REFUSED %s\n", k.name.c_str(), msg);
        return 1;
    }
    // create_classes: the tiled kernels where the sensor_map is shrunk, and on request
    const bool tiled = a.view_resize || ((c.flags & IMGENV_FLAG_VIEW_TILED) && !(c.flags & IMGENV_FLAG_VIEW_WAVE));
    std::vector<RobotClassHost> rcls;
    for (const auto& r : k.rc) {
        RobotClassHost q;
        q.shape = (int)r[0];
        for (int j = 0; j < 4; j++) q.size[j] = r[1 + j];
        q.sensor[0] = r[5];
        q.sensor[1] = r[6];
        build_robot_class(q, a.g, tiled, (c.flags & IMGENV_FLAG_AGENT_STATE_EXTRAS) != 0);
        rcls.push_back(std::move(q));
    }
    std::vector<PedClassHost> pcls;
    for (const auto& p : k.pc) {
        PedClassHost q;
        q.shape = (int)p[0];
        for (int j = 0; j < 6; j++) q.size[j] = p[1 + j];
        build_ped_class(q, a.g.res);
        pcls.push_back(std::move(q));
    }
    CreatePlan p;
    if (plan_create(c, a, Hg, Wg, k.serial, rcls, pcls, p, msg)) {
        printf("%s REFUSED %s\n", k.name.c_str(), msg);
        return 1;
    }
    PlanHandle h;  // plan_facts
    h.R = p.R; h.RL = p.RL; h.P = p.P; h.W = p.W; h.Rw = p.Rw; h.Pw = p.Pw; h.NA = p.NA;
    h.sharded = p.RL != p.R; h.sum_shard = p.layer.sum_shard; h.pow2 = p.pow2;
    h.layer = p.layer.stamp ? LAYER_STAMP : p.layer.sum ? LAYER_SUM : LAYER_COMPOSED;
    h.serial = p.serial; h.big_view = p.big_view; h.view_a4 = a.g.Wv % 4 == 0;
    h.B = a.g.B; h.lds_view = p.lds_view; h.lds_obs = p.lds_obs; h.lds_view_big = p.lds_view_big;
    h.obs_E = p.obs_E; h.n_sub = p.n_sub; h.relation = c.relation_ped_robo; h.scene = c.ped_scene_type;
    h.early = p.early;
    h.Gs = p.Gs; h.box_cells = p.box_cells;
    h.robot_classes = (int)rcls.size(); h.pack_rows = true; h.pack_bitmap_cells = 0;
    h.pack_force = k.pack < 0 ? -1 : (k.pack == 2 || k.pack == 4) ? k.pack : 0;
    for (const RobotClassHost& q : rcls) {
        const int side = 2 * q.box_rad + 1, bside = side - 4;
        h.pack_rows = h.pack_rows && !q.fp_rows.empty() && side * side <= p.box_cells;
        h.pack_bitmap_cells = std::max(h.pack_bitmap_cells, bside * bside);
    }
    h.big_full_chunks = p.big_full_chunks; h.big_bits_in_lds = p.big_bits_in_lds;
    h.crop_map = p.big_view && p.layer.stamp && p.G < ((size_t)1 << 24);  // (the byte-per-cell summary of the map, made for such handles)
    h.img_w = c.image_size[0]; h.img_h = c.image_size[1]; h.resize = p.view_resize;
    h.keep_view_maps = !(c.flags & IMGENV_FLAG_NO_VIEW_MAPS);

    auto line = [&](const char* chain, const Words& o) {
        printf("%s %s", k.name.c_str(), chain);
        for (const std::string& w : o) printf(" %s", w.c_str());
        printf("\n");
    };
    line("reset", reset_chain(h, 0));
    line("step/gates=0", step_chain(h, false, p.sfm_ahead, k.early_off, k.split_step));
    line("step/gates=1", step_chain(h, true, p.sfm_ahead, k.early_off, k.split_step));
    if (k.listed > 0 && k.listed <= p.W) line("listed", reset_chain(h, k.listed));
    return 0;
}

// ---------------------------------------------------------------------------------------- the lattice: from handle facts
static int lattice() {
    std::set<std::string> seen;
    auto take = [&](const Words& o) { seen.insert(o.begin(), o.end()); };
    // stand-ins for the class tables: a footprint box of 7 x 7 cells (a 3 x 3 bitmap), views through k_view or the tiled kernels
    const size_t lds_small = plan_lds_view(48 * 48, 364, 48), lds_large = plan_lds_view(96 * 96, 724, 96);
    if (plan_lds_bound(lds_small) || !plan_lds_bound(lds_large)) {
        printf("LATTICE: the two stand-in views no longer straddle plan_lds_bound\n");
        return 1;
    }
    const int Hg = 400, Wg = 400, n_sub = plan_n_sub(0.25);
    const int robots[] = {1, 1024, 1025, 4096, 4097, 8192, 8193}, peds[] = {0, 1, 200};
    const uint32_t flags[] = {0, IMGENV_FLAG_COMPOSE_DENSE, IMGENV_FLAG_COMPOSE_SPARSE, IMGENV_FLAG_LAYER_SUM};
    for (int RL : robots) for (int shard = 0; shard < 2; shard++) for (int P : peds) for (uint32_t fl : flags)
    for (int W : {1, 4}) for (int scene : {IMGENV_SCENE_RVO, IMGENV_SCENE_PEDSIM}) for (int big = 0; big < 2; big++) {
        const int R = shard ? 2 * RL : RL;  // (a shard: the first of two ranks)
        if (W > 1 && (shard || R % W || P % W)) continue;           // create_check_args refuses these
        if (P == 0 && scene != IMGENV_SCENE_RVO) continue;
        RobotClassHost rc = {};
        rc.shape = IMGENV_SHAPE_CIRCLE;
        rc.box_rad = 3;
        rc.big = big != 0;
        PedClassHost pc = {};
        pc.shape = IMGENV_SHAPE_CIRCLE;
        pc.box_rad = 3;
        const LayerPlan l = plan_layer_mode(R, RL, P, W, Hg, Wg, fl, {rc}, P ? std::vector<PedClassHost>{pc} : std::vector<PedClassHost>{});
        for (int pow2 = 0; pow2 < 2; pow2++) for (int a4 = 0; a4 < 2; a4++) for (int ldsb = 0; ldsb < 2; ldsb++)
        for (int pack : {-1, 2}) for (int bits = 0; bits < 2; bits++) for (int resize = 0; resize < 2; resize++) for (int cm = 0; cm < 2; cm++) {
            if (!big && (bits || resize || cm)) continue;
            if (cm && !l.stamp) continue;  // (k_crop_big reads the map's summary only beside the stamps)
            if (big && ldsb) continue;
            PlanHandle h;
            h.R = R; h.RL = RL; h.P = P; h.W = W; h.Rw = R / W; h.Pw = P / W;
            const bool rvo = scene == IMGENV_SCENE_RVO, sfm_ahead = scene == IMGENV_SCENE_PEDSIM && P > 0;  // (a crowd that ignores the robots)
            h.relation = rvo ? 1 : 0;
            h.NA = rvo && P > 0 ? P + R : 0;
            h.sharded = shard != 0; h.sum_shard = l.sum_shard; h.pow2 = pow2 != 0;
            h.layer = l.stamp ? LAYER_STAMP : l.sum ? LAYER_SUM : LAYER_COMPOSED;
            h.big_view = big != 0; h.view_a4 = a4 != 0; h.B = 360;
            h.lds_view = big ? 16 : ldsb ? lds_large : lds_small;
            h.obs_E = plan_obs_E(plan_obs_slots(h.Pw));
            h.lds_obs = plan_lds_obs(h.obs_E, plan_obs_slots(h.Pw), h.Pw);
            h.n_sub = n_sub; h.scene = P > 0 ? scene : 0;
            h.early = plan_early_obs(false, P, h.NA, sfm_ahead, false, false, h.big_view, n_sub);
            h.Gs = (size_t)Hg * Wg; h.box_cells = 49;
            h.robot_classes = 1; h.pack_rows = true; h.pack_bitmap_cells = 9; h.pack_force = pack;
            h.big_bits_in_lds = !big || bits; h.crop_map = cm != 0;
            h.img_w = h.img_h = 48; h.resize = resize != 0; h.keep_view_maps = true;
            take(reset_chain(h, 0));
            take(step_chain(h, false, sfm_ahead, false));
            take(step_chain(h, true, sfm_ahead, false));
            if (!shard) take(step_chain(h, true, sfm_ahead, false, true));
            if (W > 1) take(reset_chain(h, 2));
        }
    }
    for (const std::string& w : seen) printf("%s\n", w.c_str());
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "--lattice")) return lattice();
    std::string line;
    char buf[8192];
    int bad = 0;
    while (fgets(buf, sizeof(buf), stdin)) {
        line = buf;
        if (line.find_first_not_of(" \t\r\n") == std::string::npos) continue;
        Case k;
        if (!parse_case(line, k)) {
            printf("BAD LINE %s", buf);
            bad = 1;
            continue;
        }
        bad |= run_case(k);
    }
    return bad;
}
