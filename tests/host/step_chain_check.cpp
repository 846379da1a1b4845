// step_chain_check.cpp -- the ordering decisions of a step's chain (img_env_amd/csrc/launch_plan.h: plan_side_wiring,
// plan_snap_turn / plan_snap_in, plan_norm_chain, plan_crowd_step) and the two set helpers of sfm.h, on the CPU.
// Each decision over its whole input space against a table WRITTEN BY HAND from the code these functions replaced (launch_views
// and imgenv_step_begin as they stood before the decisions moved here: the `h->P > 0` block, the two snapshot blocks, the
// normalise tail, the block of the crowd that runs ahead) -- not printed from the functions.  Then two model runs: the crowd a step ahead, whose
// launch on its own stream must never overtake the caller's stream on the set it touches, and the snapshots' turns.
//   g++ -std=c++17 -I include tests/host/step_chain_check.cpp -o step_chain_check && ./step_chain_check
#include <stdio.h>

#include <random>

#include "../../img_env_amd/csrc/launch_plan.h"
#include "../../img_env_amd/csrc/sfm.h"

static int g_fail = 0, g_checks = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        g_checks++;                                                      \
        if (!(cond)) {                                                   \
            g_fail++;                                                    \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
        }                                                                \
    } while (0)
#define CHECK_EQ(a, b)                                                                                     \
    do {                                                                                                   \
        g_checks++;                                                                                        \
        const long long a_ = (long long)(a), b_ = (long long)(b);                                          \
        if (a_ != b_) {                                                                                    \
            g_fail++;                                                                                      \
            printf("FAIL %s:%d: %s = %lld, expected %s = %lld\n", __FILE__, __LINE__, #a, a_, #b, b_);     \
        }                                                                                                  \
    } while (0)

// ---------------------------------------------------------------------------------------- side wiring
// serial x sharded x RL 4096 / 4097 x side_reads_all x remote_only x early step, in that nesting (early innermost), a step of a
// handle with 8 RVO pedestrians.  A row: solve's stream, observation's stream (0 caller, 1 side, 2 side2), the solve's wait
// (0 none, 1 ev_fork, 2 ev_fork2), ev_fork2 recorded here, ev_fork2 on k_remote, ev_join, ev_join2.
// By hand: no side streams under IMGENV_SERIAL; one side stream (side2) up to 4096 robots of an unsharded handle, where the solve
// waits for ev_fork only in an early step; otherwise the solve on `side` behind ev_fork -- or, sharded and reading every rank's
// robots, behind ev_fork2, which k_remote carries when there is one -- and joined into the observation's stream.
static const char* const SIDE_ROWS[64] = {
    // overlap, unsharded, 4096: one side
    "2200001", "2210001", "2200001", "2210001", "2200001", "2210001", "2200101", "2210101",
    // overlap, unsharded, 4097: two sides (k_remote's event goes out even if nobody waits for it)
    "1210011", "1210011", "1210011", "1210011", "1210011", "1210011", "1210111", "1210111",
    // overlap, sharded, 4096
    "1210011", "1210011", "1210011", "1210011", "1221011", "1221011", "1220111", "1220111",
    // overlap, sharded, 4097
    "1210011", "1210011", "1210011", "1210011", "1221011", "1221011", "1220111", "1220111",
    // serial: everything on the caller's stream, no event at all
    "0000000", "0000000", "0000000", "0000000", "0000000", "0000000", "0000000", "0000000",
    "0000000", "0000000", "0000000", "0000000", "0000000", "0000000", "0000000", "0000000",
    "0000000", "0000000", "0000000", "0000000", "0000000", "0000000", "0000000", "0000000",
    "0000000", "0000000", "0000000", "0000000", "0000000", "0000000", "0000000", "0000000",
};
static void side_wiring() {
    int row = 0;
    for (int serial = 0; serial < 2; serial++)
        for (int sharded = 0; sharded < 2; sharded++)
            for (int RL = 4096; RL <= 4097; RL++)
                for (int reads_all = 0; reads_all < 2; reads_all++)
                    for (int remote_only = 0; remote_only < 2; remote_only++)
                        for (int early = 0; early < 2; early++, row++) {
                            PlanHandle h;
                            h.R = sharded ? 2 * RL : RL; h.RL = RL; h.Rw = h.R;
                            h.P = h.Pw = h.NA = 8;
                            h.relation = reads_all;
                            h.serial = serial != 0; h.sharded = sharded != 0; h.sum_shard = remote_only != 0;
                            PlanChain c;
                            c.act_nw = 1; c.act_ng = h.R; c.act_nl = RL; c.act_np = 8;
                            const SidePlan s = plan_side(h, c);
                            CHECK_EQ(s.side_reads_all, reads_all);
                            CHECK_EQ(s.remote_only, remote_only);
                            const SideWiring w = plan_side_wiring(s, h, early != 0);
                            const char* e = SIDE_ROWS[row];
                            CHECK_EQ(w.solve_on, e[0] - '0');
                            CHECK_EQ(w.obs_on, e[1] - '0');
                            CHECK_EQ(w.solve_waits, e[2] - '0');
                            CHECK_EQ(w.record_fork2, e[3] - '0');
                            CHECK_EQ(w.fork2_on_remote, e[4] - '0');
                            CHECK_EQ(w.join, e[5] - '0');
                            CHECK_EQ(w.join2, e[6] - '0');
                            // an event somebody waits for goes out exactly once; what is recorded on the caller's stream is waited for
                            if (w.solve_waits == WAIT_FORK2) CHECK(w.record_fork2 != w.fork2_on_remote);
                            if (w.record_fork2) CHECK_EQ(w.solve_waits, WAIT_FORK2);
                        }
    CHECK_EQ(row, 64);
    CHECK_EQ(ON_CALLER, 0); CHECK_EQ(ON_SIDE, 1); CHECK_EQ(ON_SIDE2, 2);
    CHECK_EQ(WAIT_NONE, 0); CHECK_EQ(WAIT_FORK, 1); CHECK_EQ(WAIT_FORK2, 2);
    // a handle without pedestrians has no side launches whatever else it is
    PlanHandle h;
    h.R = h.RL = h.Rw = 14;
    PlanChain c;
    c.act_nw = 1; c.act_ng = c.act_nl = 14;
    const SideWiring w = plan_side_wiring(plan_side(h, c), h, false);
    CHECK_EQ(w.solve_on, ON_CALLER); CHECK_EQ(w.obs_on, ON_CALLER); CHECK_EQ(w.solve_waits, WAIT_NONE);
    CHECK(!w.record_fork2 && !w.fork2_on_remote && !w.join && !w.join2);
}

// ---------------------------------------------------------------------------------------- snapshot turn
// By hand: out = buffer[seq & 1] on a handle that can run early steps, out2 = buffer[(seq + 1) & 1] only for a listed launch, the
// sequence advances unless listed; an early step reads buffer[(seq - 1) & 1].
static void snapshot_turn() {
    struct Row { unsigned seq; int early, listed, out, out2, advance; };
    const unsigned last = 0u - 1;
    static const Row rows[] = {
        {0, 0, 0, -1, -1, 1}, {0, 0, 1, -1, -1, 0}, {0, 1, 0, 0, -1, 1}, {0, 1, 1, 0, 1, 0},
        {1, 0, 0, -1, -1, 1}, {1, 0, 1, -1, -1, 0}, {1, 1, 0, 1, -1, 1}, {1, 1, 1, 1, 0, 0},
        {2, 0, 0, -1, -1, 1}, {2, 0, 1, -1, -1, 0}, {2, 1, 0, 0, -1, 1}, {2, 1, 1, 0, 1, 0},
        {7, 0, 0, -1, -1, 1}, {7, 0, 1, -1, -1, 0}, {7, 1, 0, 1, -1, 1}, {7, 1, 1, 1, 0, 0},
        {last, 0, 0, -1, -1, 1}, {last, 0, 1, -1, -1, 0}, {last, 1, 0, 1, -1, 1}, {last, 1, 1, 1, 0, 0},
    };
    for (const Row& r : rows) {
        const SnapTurn t = plan_snap_turn(r.seq, r.early != 0, r.listed != 0);
        CHECK_EQ(t.out, r.out); CHECK_EQ(t.out2, r.out2); CHECK_EQ(t.advance, r.advance);
    }
    CHECK_EQ(plan_snap_in(0), 1); CHECK_EQ(plan_snap_in(1), 0); CHECK_EQ(plan_snap_in(2), 1); CHECK_EQ(plan_snap_in(7), 0);
    CHECK_EQ(plan_snap_in(last), 0);
    // a run across the wrap: steps (early ones from the second launch on) with listed reset chains scattered in between.  The buffer
    // an early step's k_obs reads is never the one its own chain's launch writes, and it is the one the last launch wrote (a step's
    // out, or both buffers behind a listed launch); a listed launch writes both buffers and leaves the sequence alone.
    // (`in != out` alone holds for any sequence number by the two formulas; what catches a wrong turn -- a launch that advances when
    // it should not, or does not when it should -- is the tracking of the buffer the last launch really wrote.)
    std::mt19937 rng(20240607u);
    unsigned seq = 0u - 40;
    int last_written = -1;  // -1: nothing yet, 2: both
    for (int step = 0; step < 400; step++) {
        if (rng() % 5 == 0) {
            const unsigned before = seq;
            const SnapTurn t = plan_snap_turn(seq, true, true);
            CHECK(t.out >= 0 && t.out2 >= 0 && t.out != t.out2);
            if (t.advance) seq += 1;
            CHECK_EQ(seq, before);
            last_written = 2;
        }
        const int in = last_written >= 0 ? plan_snap_in(seq) : -1;  // (plan_step: no early step before a first launch)
        const SnapTurn t = plan_snap_turn(seq, true, false);
        CHECK_EQ(t.out2, -1);
        if (in >= 0) {
            CHECK(in != t.out);
            CHECK(last_written == 2 || last_written == in);
        }
        CHECK(t.advance);
        seq += 1;
        last_written = t.out;
    }
    CHECK(seq < 400u);  // (the run crossed the wrap)
}

// ---------------------------------------------------------------------------------------- normalise chain
// training x reward flag x n_obs 0 / 3 x reset chain -> n_ret, cols, update, k_norm_part, k_norm_apply, norm_turn, norm_ret_turn.
// By hand: a reset chain has no return column; the statistics move with training on unless a reset chain has no observed column;
// the apply runs unless a reset chain has nothing observed and no return to restart (training && reward).
static void normalise_chain() {
    static const int rows[16][11] = {
        {0, 0, 0, 0, /**/ 0, 1, 0, 0, 1, 0, 0}, {0, 0, 0, 1, /**/ 0, 1, 0, 0, 0, 0, 0},
        {0, 0, 3, 0, /**/ 0, 3, 0, 0, 1, 0, 0}, {0, 0, 3, 1, /**/ 0, 3, 0, 0, 1, 0, 0},
        {0, 1, 0, 0, /**/ 1, 1, 0, 0, 1, 0, 0}, {0, 1, 0, 1, /**/ 0, 1, 0, 0, 0, 0, 0},
        {0, 1, 3, 0, /**/ 1, 4, 0, 0, 1, 0, 0}, {0, 1, 3, 1, /**/ 0, 3, 0, 0, 1, 0, 0},
        {1, 0, 0, 0, /**/ 0, 1, 1, 1, 1, 1, 0}, {1, 0, 0, 1, /**/ 0, 1, 1, 0, 0, 0, 0},
        {1, 0, 3, 0, /**/ 0, 3, 1, 1, 1, 1, 0}, {1, 0, 3, 1, /**/ 0, 3, 1, 1, 1, 1, 0},
        {1, 1, 0, 0, /**/ 1, 1, 1, 1, 1, 1, 1}, {1, 1, 0, 1, /**/ 0, 1, 1, 0, 1, 0, 0},
        {1, 1, 3, 0, /**/ 1, 4, 1, 1, 1, 1, 1}, {1, 1, 3, 1, /**/ 0, 3, 1, 1, 1, 1, 0},
    };
    for (const auto& r : rows) {
        const NormChain n = plan_norm_chain(r[0] != 0, r[1] != 0, r[2], r[3] != 0);
        CHECK_EQ(n.n_ret, r[4]); CHECK_EQ(n.cols, r[5]); CHECK_EQ(n.update, r[6]); CHECK_EQ(n.part, r[7]); CHECK_EQ(n.apply, r[8]);
        CHECK_EQ(n.turn, r[9]); CHECK_EQ(n.ret_turn, r[10]);
    }
}

// ---------------------------------------------------------------------------------------- crowd step
// CrowdAhead: can x valid x steps_since_reset 0 / 1 / 2 x par -> swap, the ev_in left, the one the launch ahead
// waits for (-1: none), the next parity.  By hand: a handle that cannot run ahead steps in place and leaves nothing; otherwise
// the step leaves ev_in[par] and flips the parity, swaps iff the other set is valid, and from the second step behind a reset
// on the launch ahead waits for the last step's event (par ^ 1) behind a swap, for this step's own (par) behind a step in place.
static void crowd_step_table() {
    static const int rows[24][8] = {
        {0, 0, 0, 0, /**/ 0, -1, -1, 0}, {0, 0, 0, 1, /**/ 0, -1, -1, 1}, {0, 0, 1, 0, /**/ 0, -1, -1, 0}, {0, 0, 1, 1, /**/ 0, -1, -1, 1},
        {0, 0, 2, 0, /**/ 0, -1, -1, 0}, {0, 0, 2, 1, /**/ 0, -1, -1, 1}, {0, 1, 0, 0, /**/ 0, -1, -1, 0}, {0, 1, 0, 1, /**/ 0, -1, -1, 1},
        {0, 1, 1, 0, /**/ 0, -1, -1, 0}, {0, 1, 1, 1, /**/ 0, -1, -1, 1}, {0, 1, 2, 0, /**/ 0, -1, -1, 0}, {0, 1, 2, 1, /**/ 0, -1, -1, 1},
        {1, 0, 0, 0, /**/ 0, 0, -1, 1}, {1, 0, 0, 1, /**/ 0, 1, -1, 0}, {1, 0, 1, 0, /**/ 0, 0, 0, 1}, {1, 0, 1, 1, /**/ 0, 1, 1, 0},
        {1, 0, 2, 0, /**/ 0, 0, 0, 1}, {1, 0, 2, 1, /**/ 0, 1, 1, 0}, {1, 1, 0, 0, /**/ 1, 0, -1, 1}, {1, 1, 0, 1, /**/ 1, 1, -1, 0},
        {1, 1, 1, 0, /**/ 1, 0, 1, 1}, {1, 1, 1, 1, /**/ 1, 1, 0, 0}, {1, 1, 2, 0, /**/ 1, 0, 1, 1}, {1, 1, 2, 1, /**/ 1, 1, 0, 0},
    };
    for (const auto& r : rows) {
        const CrowdStep k = plan_crowd_step(r[0] != 0, r[1] != 0, r[2], r[3]);
        CHECK_EQ(k.swap, r[4]); CHECK_EQ(k.leaves, r[5]); CHECK_EQ(k.ahead_waits, r[6]); CHECK_EQ(k.par_next, r[7]);
    }
}

// The model run.  Two sets of the eight arrays a step writes (real SfmDev records with made-up addresses, moved by sfm_swap_sets
// and sfm_write_into as the host code moves them); a clock that ticks once per operation on the caller's stream; per set the tick
// of the caller's stream's last access and last write; per ev_in the tick (and step) that recorded it.  Steps as
// imgenv_step_begin takes them, resets (sfm_ahead_drop + a write to the live set on the caller's stream) scattered by a fixed
// seed, and behind each the steps in place that follow from it.  What must hold for every launch ahead:
//   it writes the set that is NOT live, and waits for an event recorded at or after the caller's stream's last access to it
//   (the first "high" finding of ADVICE.md: the crowd's stream overwrote a set the caller's stream had not published yet);
//   it reads the live set, and waits for an event recorded at or after the caller's stream's last write to that.
// `rule` decides; the run counts violations, so that a wrong rule can be shown to be caught.
typedef CrowdStep (*CrowdRule)(bool, bool, int, int);
static CrowdStep rule_last_step_always(bool ahead, bool valid, int since, int par) {  // (wrong behind a step in place)
    CrowdStep k = plan_crowd_step(ahead, valid, since, par);
    if (k.ahead_waits >= 0) k.ahead_waits = par ^ 1;
    return k;
}
static CrowdStep rule_own_always(bool ahead, bool valid, int since, int par) {  // (right, but gives up the step of slack)
    CrowdStep k = plan_crowd_step(ahead, valid, since, par);
    if (k.ahead_waits >= 0) k.ahead_waits = par;
    return k;
}
struct SetArrays { double p[1], v[1]; int dq[1], dest[1], last[1], n_nodes[1], treehash[1]; SfmNode nodes[1]; };
static int set_of(const SetArrays* sets, const double* p) { return p == sets[0].p ? 0 : p == sets[1].p ? 1 : -1; }
static bool writes_set(const SfmDev& f, const SetArrays& s) {
    return f.p_out == s.p && f.v_out == s.v && f.dq_out == s.dq && f.dest_out == s.dest && f.last_out == s.last && f.nodes_out == s.nodes &&
           f.n_nodes_out == s.n_nodes && f.treehash_out == s.treehash;
}
static bool holds_set(const SfmDev& f, const SetArrays& s) {
    return f.p == s.p && f.v == s.v && f.dq == s.dq && f.dest == s.dest && f.last == s.last && f.nodes == s.nodes && f.n_nodes == s.n_nodes &&
           f.treehash == s.treehash;
}
static int crowd_model(CrowdRule rule, unsigned seed, int steps, int* launches_ahead, int* in_place_steps) {
    static SetArrays sets[2];
    SfmDev live = {}, other = {};
    SfmDev* both[2] = {&live, &other};
    for (int q = 0; q < 2; q++) {
        SfmDev& f = *both[q];
        f.p = sets[q].p; f.v = sets[q].v; f.dq = sets[q].dq; f.dest = sets[q].dest; f.last = sets[q].last;
        f.nodes = sets[q].nodes; f.n_nodes = sets[q].n_nodes; f.treehash = sets[q].treehash;
    }
    sfm_write_into(live, live);
    std::mt19937 rng(seed);
    bool valid = false;
    int since = 0, par = 0, violations = 0;
    long tick = 0, access[2] = {0, 0}, write[2] = {0, 0}, ev_tick[2] = {-1, -1};
    int ev_step[2] = {-1, -1};
    for (int step = 0; step < steps; step++) {
        if (step == 0 || rng() % 7 == 0) {  // a reset: drops what was computed ahead, then writes the live crowd on the caller's stream
            valid = false;
            since = 0;
            const int l = set_of(sets, live.p);
            access[l] = write[l] = ++tick;
        }
        const CrowdStep k = rule(true, valid, since, par);
        CHECK(!valid || since >= 1);  // (a launch ahead has gone out since the reset)
        par = k.par_next;
        ++tick;
        if (k.swap) {  // the publish reads the set that becomes live
            sfm_swap_sets(live, other);
            sfm_write_into(live, live);
            access[set_of(sets, live.p)] = tick;
        } else {  // k_sfm in place
            access[set_of(sets, live.p)] = write[set_of(sets, live.p)] = tick;
            *in_place_steps += 1;
        }
        const int l = set_of(sets, live.p), o = set_of(sets, other.p);
        CHECK(l >= 0 && o >= 0 && l != o);
        CHECK(holds_set(live, sets[l]) && holds_set(other, sets[o]) && writes_set(live, sets[l]));
        CHECK(k.leaves == 0 || k.leaves == 1);
        ev_tick[k.leaves] = tick;
        ev_step[k.leaves] = step;
        since += 1;
        if (k.ahead_waits < 0) continue;
        SfmDev launch = live;  // (launch_sfm: a copy of the live record that writes the other set)
        sfm_write_into(launch, other);
        CHECK(holds_set(launch, sets[l]) && writes_set(launch, sets[o]));
        *launches_ahead += 1;
        const int w = k.ahead_waits;
        CHECK(ev_step[w] == step || ev_step[w] == step - 1);
        if (ev_tick[w] < access[o] || ev_tick[w] < write[l]) violations++;
        valid = true;
    }
    return violations;
}
static void crowd_model_runs() {
    int ahead = 0, in_place = 0, x = 0, y = 0;
    for (unsigned seed = 1; seed <= 4; seed++) CHECK_EQ(crowd_model(plan_crowd_step, seed, 400, &ahead, &in_place), 0);
    CHECK(ahead > 800 && in_place > 300);  // (both kinds of step happened, often)
    CHECK_EQ(crowd_model(rule_own_always, 1, 400, &x, &y), 0);
    CHECK(crowd_model(rule_last_step_always, 1, 400, &x, &y) > 0);  // (the model sees a wrong rule)
}

int main() {
    side_wiring();
    snapshot_turn();
    normalise_chain();
    crowd_step_table();
    crowd_model_runs();
    if (g_fail) {
        printf("%d of %d checks failed\n", g_fail, g_checks);
        return 1;
    }
    printf("OK %d checks\n", g_checks);
    return 0;
}
