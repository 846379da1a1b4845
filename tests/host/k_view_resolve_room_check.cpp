// CPU model of the bookkeeping of k_view's step (5) (img_env_amd/csrc/kernels.h, "the cells a top beam left alone"), without a GPU.
// The step resolves those cells in three scratch areas carved out of dead LDS -- the skip list, cap_d chunk descriptors behind it,
// cap_r result slots in the column table (launch_plan.h: plan_resolve_room) -- and a cell that finds no room walks its list alone.
// Per view occupancy this program
//   1. builds the class with build_robot_class, computes hit words and the reach table as k_view_tables_check.cpp does, walks the
//      group list of a reset (all_groups) or of a step (dyn_groups) as the kernel's final pass does and reports: n_skip (list entries),
//      flagged cells, cells passing the reach filter, descriptors wanted (sum of nch), slots wanted (cells of several chunks),
//      cap_d, cap_r;
//   2. replays A / B / C of the step sequentially, in the allocation order of the one-wavefront variant, with the caps as
//      PARAMETERS -- the product's, the tiny build's (5, 2), (0, 0), and each area short on its own -- with the kernel's own
//      packing of descriptors, slots and atomicMin keys, every array bounds-checked and poisoned, and demands that each
//      laser_map equals the reference's sequential beam-after-beam algorithm (own footprint stamped);
//   3. checks that every packed field fits its bits at this geometry: slot < 1024, cell < 65535, list position <= 4095, chunk
//      entries - 1 <= 7, first entry < 2^20, and that the product caps fit the LDS they are carved from.
// usage: k_view_resolve_room_check <view_w> <view_h> <res> <beams> <angle_begin> <angle_end> <min_dist> <max_dist> <radius> <n_robots> scenes <seed>
//        ... file <path>      path: int32 n_views, int32 NC, n_views bytes (1: a reset's pass, 0: a step's), n_views x NC bytes (non-zero: occupied)
// prints  GEOM Hv Wv B NC lds_view lds_bound nw a4      (plan_lds_view / plan_lds_bound / plan_views for a launch of n_robots)
//         S <scene> <n_skip> <flagged> <passing> <need_d> <cap_d> <need_r> <cap_r> <alone_r>     (scenes)
//         V <view> <n_skip> <flagged> <passing> <need_d> <cap_d> <need_r> <cap_r> <alone_r>      (file)
//           alone_r: cells that walk alone with the product caps for want of a slot although their descriptors had room
//         OK ...                                                                       exit code 0 = all good
#include <stdio.h>

#include <random>
#include <string>

#define WAVE_SZ 64
#include "../../img_env_amd/csrc/host_tables.h"

static int fail(const char* what, long a = 0, long b = 0, long c = 0) {
    printf("FAIL %s (%ld %ld %ld)\n", what, a, b, c);
    return 1;
}

struct Counts {
    int n_skip = 0, flagged = 0, passing = 0, need_d = 0, need_r = 0, cap_d = 0, cap_r = 0;
    int alone_r = 0;  // cells that walk alone with the product caps although their descriptors had room: for want of a slot
};

struct Model {
    RobotClassHost k;
    ViewGeom g;
    int Hv, Wv, NC, B, S;
    std::vector<std::vector<int>> path;
    uint32_t lvl_n[3], lvl_off[3];
    const char* why = "";
    long w0 = 0, w1 = 0, w2 = 0;

    bool err(const char* what, long a = 0, long b = 0, long c = 0) {
        why = what; w0 = a; w1 = b; w2 = c;
        return false;
    }
    bool stamped(int c) const { return ((k.stamp_bits[c >> 5] >> (c & 31)) & 1u) != 0u; }
    bool in_fov(int c) const { return ((k.fov_bits[c >> 5] >> (c & 31)) & 1u) != 0u; }

    // patch_stamped of kernels.h on class indices (0 -> 0, 1 -> 100, 2 -> 200, 3 -> 255)
    static void patch(std::vector<uint8_t>& out, uint32_t c, uint32_t v, bool st) {
        if (v == 2u) return;
        out[c] = (uint8_t)((st && v != 0u) ? 1u : v);
    }
    // resolve_skipped_cell of kernels.h
    uint32_t walk_alone(const std::vector<uint32_t>& hit, uint32_t c) const {
        const uint32_t pk = k.inv_pack[c], e0 = pk & 0xFFFFFu, cnt = pk >> 20;
        for (uint32_t e = 1; e < cnt; e++) {
            const uint32_t ent = k.inv_ent[e0 + e], kk = ent & 0xFFFFu, hp = hit[ent >> 16], hk = hp >> 16;
            if (kk < hk) return 3u;
            if (kk == hk) return 0u;
            if (kk > (hp & 0xFFFFu)) break;
        }
        return 2u;
    }

    // one view: occ[c] != 0 = the crop holds an occupied cell (cells outside the field of view never do); reset: the pass over every group.
    // caps[][2]: (cap_d, cap_r) settings to replay, -1 = the product's
    bool run(const std::vector<uint8_t>& occ_in, bool reset, Counts& n, const int (*caps)[2], int n_caps) {
        std::vector<uint8_t> occ(NC);
        for (int c = 0; c < NC; c++) occ[c] = occ_in[c] != 0 && in_fov(c);
        std::vector<int> hk(B, -1);
        for (int b = 0; b < B; b++)
            for (int q = 0; q < (int)path[b].size(); q++)
                if (occ[path[b][q]]) { hk[b] = q; break; }
        // reference: beams in order, later beams overwrite earlier ones (agent.cpp:419-437, 511-624), then the own footprint (agent.cpp:503)
        std::vector<uint8_t> ref(NC, 2);
        for (int b = 0; b < B; b++)
            for (int q = 0; q < (int)path[b].size(); q++) {
                const int cc = path[b][q];
                if (hk[b] < 0 || q < hk[b]) ref[cc] = 3;
                else if (q == hk[b]) ref[cc] = 0;
                else {
                    const int hx = path[b][hk[b]] / Wv, hy = path[b][hk[b]] % Wv;
                    if (cc / Wv == hx || cc % Wv == hy) continue;
                    ref[cc] = 2;
                }
            }
        for (int c = 0; c < NC; c++)
            if (stamped(c) && ref[c] != 0) ref[c] = 1;
        // hit words and the reach table (kernels.h phase (3))
        std::vector<uint32_t> hit(B + 1);
        for (int b = 0; b < B; b++) hit[b] = hk[b] < 0 ? 0xFFFFFFFFu : (((uint32_t)hk[b] << 16) | (uint32_t)(hk[b] + k.ray_run[(size_t)hk[b] * S + b]));
        hit[B] = 0;
        std::vector<uint32_t> reach(lvl_off[2] + lvl_n[2]);
        for (uint32_t i = 0; i < lvl_n[0]; i++) {
            uint32_t m = 0;
            for (int q = 0; q < 16; q++) m = std::max(m, hit[std::min<uint32_t>(8 * i + q, B)]);
            reach[i] = m;
        }
        for (uint32_t i = 0; i < lvl_n[1]; i++) reach[lvl_off[1] + i] = std::max(reach[2 * i], reach[std::min(2 * i + 2, lvl_n[0] - 1)]);
        for (uint32_t i = 0; i < lvl_n[2]; i++) reach[lvl_off[2] + i] = std::max(reach[lvl_off[1] + 2 * i], reach[lvl_off[1] + std::min(2 * i + 2, lvl_n[1] - 1)]);
        // (4) the final pass over the group list: provisional classes and the skip list (one entry per group with a flagged cell, in
        // list order).  The cells of groups a step does not list hold their 200 / 100 since the reset.
        std::vector<uint8_t> base(NC);
        for (int c = 0; c < NC; c++) base[c] = stamped(c) ? 1 : 2;
        const std::vector<uint32_t>& glist = reset ? k.all_groups : k.dyn_groups;
        const uint32_t no_beam = ((uint32_t)B << 16) | 0xFFFFu;
        std::vector<uint32_t> skip_list;
        for (uint32_t g_cur : glist) {
            const int c4 = (int)(g_cur & 0xFFFFu);
            uint32_t skips = 0;
            for (int q = 0; q < 4 && c4 + q < NC; q++) {
                const uint32_t top = k.top_ent[c4 + q], kk = top & 0xFFFFu, hp = hit[top >> 16], h = hp >> 16;
                uint32_t v = top == no_beam ? 2u : (kk < h ? 3u : (kk == h ? 0u : 2u));
                if (top != no_beam && kk > h && kk <= (hp & 0xFFFFu)) skips |= 1u << q;
                if (((g_cur >> (20 + q)) & 1u) != 0u && v != 0u) v = 1u;
                base[c4 + q] = (uint8_t)v;
            }
            if (skips) skip_list.push_back(((uint32_t)c4 << 4) | skips);
        }
        const int n_skip = (int)skip_list.size();
        const int NCp = (NC + 16) & ~15, n_even = (n_skip + 1) & ~1;
        if (n_skip > NCp / 4) return err("the skip list does not fit the dead crop", n_skip, NCp / 4);
        const ResolveRoom room = plan_resolve_room(NC, Wv, n_skip);
        if (room.cap_d < 0 || n_even + 2 * room.cap_d > NCp / 4) return err("product cap_d does not fit behind the skip list", room.cap_d, n_even, NCp / 4);
        if (room.cap_r > 4 * Wv || room.cap_r > 1024) return err("product cap_r does not fit the column table / 10 bits", room.cap_r);
        n = Counts();
        n.n_skip = n_skip;
        n.cap_d = room.cap_d;
        n.cap_r = room.cap_r;
        for (int s = 0; s < n_caps; s++) {
            const int cap_d = caps[s][0] < 0 ? room.cap_d : caps[s][0], cap_r = caps[s][1] < 0 ? room.cap_r : caps[s][1];
            const uint32_t POISON = 0xDEADBEEFu;
            std::vector<uint32_t> desc_x(cap_d, POISON), desc_y(cap_d, POISON), slots(cap_r, POISON);
            std::vector<uint8_t> out(base);
            int flagged = 0, passing = 0, alone_r = 0;
            int base_d = 0, base_r = 0;  // the one-wavefront variant's cursors: a running prefix sum over the items in order
            for (int t = 0; t < 4 * n_skip; t++) {  // A
                const uint32_t e = skip_list[t >> 2], q = (uint32_t)t & 3u;
                if (((e >> q) & 1u) == 0u) continue;
                const uint32_t c = (e >> 4) + q;
                if ((int)c >= NC) return err("flagged cell beyond the view", c);
                flagged++;
                const uint32_t f = k.inv_cell[2 * (size_t)c], pk = k.inv_cell[2 * (size_t)c + 1];
                const uint32_t nn = (pk >> 20) - 1u, nch = (nn + 7u) >> 3;
                const bool st = ((f >> 14) & 1u) != 0u;
                const bool pass = nch != 0u && (((f >> 13) & 1u) != 0u || (reach[f & 0x1FFFu] >> 16) >= (f >> 24));
                if (!pass) {
                    if (walk_alone(hit, c) != 2u) return err("the reach filter dropped a cell that changes", c);
                    continue;
                }
                passing++;
                const bool multi = nch > 1u;
                const int pos = base_d, slot = base_r;
                base_d += (int)nch;
                base_r += multi ? 1 : 0;
                if (nn > 4095u) return err("list position beyond 12 bits", c, nn);
                const bool alone = pos + (int)nch > cap_d || (multi && slot >= cap_r);
                if (alone && pos + (int)nch <= cap_d) alone_r++;
                const uint32_t e0 = pk & 0xFFFFFu;
                if (multi && slot < cap_r) slots[slot] = ((uint32_t)st << 30) | (0xFFFu << 18) | (2u << 16) | c;
                if (!alone) {
                    if (multi && slot >= 1024) return err("slot beyond 10 bits", c, slot);
                    if (c >= 0xFFFFu) return err("cell beyond 16 bits", c);
                    if (e0 + 1u + 8u * (nch - 1u) >= (1u << 20) || nch - 1u >= (1u << 12)) return err("first entry / chunk number beyond their bits", c, e0, nch);
                }
                const uint32_t lo = c | ((uint32_t)slot << 19) | ((uint32_t)st << 29) | (multi ? 0u : 0x80000000u);
                for (int j = 0; j < (int)nch && pos + j < cap_d; j++) {
                    const uint32_t ents = std::min(8u, nn - 8u * (uint32_t)j) - 1u;
                    if (ents > 7u) return err("chunk entries - 1 beyond 3 bits", c, j, ents);
                    if (pos + j < 0 || pos + j >= (int)desc_x.size()) return err("A writes a descriptor out of bounds", c, pos + j, cap_d);
                    desc_x[pos + j] = alone ? 0xFFFFFFFFu : (lo | (ents << 16));
                    desc_y[pos + j] = alone ? 0u : ((e0 + 1u + 8u * (uint32_t)j) | ((uint32_t)j << 20));
                }
                if (alone) patch(out, c, walk_alone(hit, c), st);
            }
            if (s == 0) {
                n.flagged = flagged;
                n.passing = passing;
                n.need_d = base_d;
                n.need_r = base_r;
                n.alone_r = alone_r;
            }
            const int nd = std::min(base_d, cap_d), nr = std::min(base_r, cap_r);
            if (nd > (int)desc_x.size() || nr > (int)slots.size()) return err("B / C run beyond their areas", nd, nr);
            for (int t = 0; t < nd; t++) {  // B
                if (desc_x[t] == POISON && desc_y[t] == POISON) return err("B reads a descriptor nobody wrote", t, nd, cap_d);
                const uint32_t dx = desc_x[t], dy = desc_y[t], c = dx & 0xFFFFu;
                if (c == 0xFFFFu) continue;
                const uint32_t nv = (dx >> 16) & 7u, first = dy & 0xFFFFFu, eb = 1u + 8u * (dy >> 20);
                uint32_t key = 0xFFFFFFFFu;
                for (uint32_t q = 0; q < 8; q++) {
                    const size_t at = first + std::min(q, nv);
                    if (at >= k.inv_ent.size()) return err("B reads beyond the ray lists", t, (long)at);
                    const uint32_t ent = k.inv_ent[at], kk = ent & 0xFFFFu, hp = hit[ent >> 16], h = hp >> 16;
                    const uint32_t v = kk < h ? 3u : (kk == h ? 0u : 2u);
                    const bool decides = !((kk > h) && (kk <= (hp & 0xFFFFu))) && q <= nv;
                    if (decides && eb + q > 4095u) return err("list position beyond the key's 12 bits", c, eb + q);
                    key = std::min(key, decides ? (((eb + q) << 18) | (v << 16)) : 0xFFFFFFFFu);
                }
                if (key != 0xFFFFFFFFu) {
                    if ((dx >> 31) != 0u) patch(out, c, (key >> 16) & 3u, ((dx >> 29) & 1u) != 0u);
                    else {
                        const uint32_t sl = (dx >> 19) & 0x3FFu;
                        if ((int)sl >= cap_r || slots[sl] == POISON) return err("B writes a slot nobody owns", t, sl, cap_r);
                        if ((slots[sl] & 0xFFFFu) != c) return err("B writes another cell's slot", t, sl, c);
                        slots[sl] = std::min(slots[sl], key | c | (((dx >> 29) & 1u) << 30));
                    }
                }
            }
            for (int t = 0; t < nr; t++) {  // C
                const uint32_t key = slots[t];
                if (key == POISON) return err("C reads a slot nobody wrote", t, nr);
                if ((key & 0xFFFFu) >= (uint32_t)NC) return err("C patches a cell beyond the view", t, key & 0xFFFFu);
                patch(out, key & 0xFFFFu, (key >> 16) & 3u, ((key >> 30) & 1u) != 0u);
            }
            for (int c = 0; c < NC; c++)
                if (out[c] != ref[c]) return err("laser_map", s, c, out[c] * 10 + ref[c]);
        }
        return true;
    }
};

int main(int argc, char** argv) {
    if (argc < 13) return fail("usage");
    imgenv_cfg c;
    memset(&c, 0, sizeof(c));
    c.view_width = (float)atof(argv[1]);
    c.view_height = (float)atof(argv[2]);
    c.view_resolution = (float)atof(argv[3]);
    c.use_laser = 1;
    c.range_total = atoi(argv[4]);
    c.view_angle_begin = (float)atof(argv[5]);
    c.view_angle_end = (float)atof(argv[6]);
    c.view_min_dist = (float)atof(argv[7]);
    c.view_max_dist = (float)atof(argv[8]);
    const int n_robots = atoi(argv[10]);
    const std::string mode = argv[11];
    Model m;
    m.g = make_view_geom(c);
    m.k.shape = IMGENV_SHAPE_CIRCLE;
    m.k.size[0] = 0.f; m.k.size[1] = 0.f; m.k.size[2] = (float)atof(argv[9]); m.k.size[3] = 0.f;
    m.k.sensor[0] = 0.f; m.k.sensor[1] = 0.f;
    build_robot_class(m.k, m.g);
    if (!m.k.ok) return fail("class tables overflow");
    if (m.k.big) return fail("a big class: not k_view's");
    m.Hv = m.g.Hv; m.Wv = m.g.Wv; m.NC = m.Hv * m.Wv; m.B = m.g.B; m.S = m.k.ray_stride;
    const int Hv = m.Hv, Wv = m.Wv, NC = m.NC, B = m.B;
    m.path.resize(B);
    for (int b = 0; b < B; b++)
        for (int q = 0; q < m.k.ray_len[b]; q++) m.path[b].push_back(m.k.ray_rows[((q / 8) * (size_t)m.S + b) * 8 + (q % 8)]);
    const uint32_t nb8 = ((uint32_t)B >> 3) + 1;
    m.lvl_n[0] = nb8; m.lvl_n[1] = (nb8 + 1) >> 1; m.lvl_n[2] = (nb8 + 3) >> 2;
    m.lvl_off[0] = 0; m.lvl_off[1] = m.lvl_n[0]; m.lvl_off[2] = m.lvl_n[0] + m.lvl_n[1];
    // the bit widths that hold for every occupancy of this geometry
    if (NC >= 0xFFFF) return fail("cell beyond 16 bits", NC);
    if (plan_resolve_room(NC, Wv, 0).cap_r > 1024) return fail("slot beyond 10 bits", plan_resolve_room(NC, Wv, 0).cap_r);
    for (int q = 0; q < NC; q++)
        if ((m.k.inv_pack[q] >> 20) > 4096u) return fail("list position beyond 12 bits", q, m.k.inv_pack[q] >> 20);
    {   // the launch shape of a handle with this view, as imgenv_create and launch_views derive it
        PlanHandle h;
        PlanChain ch;
        h.lds_view = plan_lds_view((size_t)NC, (size_t)m.S + 4, Wv);
        h.RL = h.R = ch.act_nl = n_robots;
        const ViewPlan v = plan_views(h, ch);
        printf("GEOM %d %d %d %d %zu %d %d %d\n", Hv, Wv, B, NC, h.lds_view, v.lds_bound ? 1 : 0, v.nw, Wv % 4 == 0 ? 1 : 0);
    }
    // the product's, the tiny build's, none at all; then each area short on its own: slots alone, descriptors alone
    const int N_CAPS = 5, caps[N_CAPS][2] = {{-1, -1}, {5, 2}, {0, 0}, {1 << 13, 2}, {5, 1024}};
    long n_views = 0;
    if (mode == "scenes") {
        const unsigned seed = (unsigned)atoi(argv[12]);
        const int sx = m.k.sensor_x, sy = m.k.sensor_y;
        std::mt19937 rng(seed);
        auto show = [&](const char* name, const std::vector<uint8_t>& occ) {
            for (int reset = 0; reset < 2; reset++) {
                Counts n;
                if (!m.run(occ, reset != 0, n, caps, N_CAPS)) {
                    printf("FAIL %s in scene %s (%ld %ld %ld)\n", m.why, name, m.w0, m.w1, m.w2);
                    return false;
                }
                if (reset) printf("S %s %d %d %d %d %d %d %d %d\n", name, n.n_skip, n.flagged, n.passing, n.need_d, n.cap_d, n.need_r, n.cap_r, n.alone_r);
                n_views++;
            }
            return true;
        };
        // the idealised scenes, centred on the sensor cell
        for (int d = 1; d <= 3; d++) {
            std::vector<uint8_t> occ(NC, 0);
            for (int a = 0; a < Hv; a++)
                for (int b = 0; b < Wv; b++)
                    if (std::max(abs(a - sx), abs(b - sy)) == d) occ[a * Wv + b] = 1;
            if (!show(d == 1 ? "ring1" : d == 2 ? "ring2" : "ring3", occ)) return 1;
        }
        {
            std::vector<uint8_t> occ(NC, 0);
            for (int b = 0; b < Wv; b++)
                for (int a : {sx - 1, sx + 1})
                    if (a >= 0 && a < Hv) occ[a * Wv + b] = 1;
            if (!show("row_walls", occ)) return 1;
        }
        {
            std::vector<uint8_t> occ(NC, 0);
            for (int a = 0; a < Hv; a++)
                for (int b : {sy - 1, sy + 1})
                    if (b >= 0 && b < Wv) occ[a * Wv + b] = 1;
            if (!show("col_walls", occ)) return 1;
        }
        for (int pct : {5, 30}) {
            std::vector<uint8_t> occ(NC, 0);
            for (int q = 0; q < NC; q++) occ[q] = (int)(rng() % 100) < pct && q != sx * Wv + sy;
            if (!show(pct == 5 ? "random5" : "random30", occ)) return 1;
        }
        {
            std::vector<uint8_t> occ(NC, 0);
            for (int q = 0; q < NC; q++) occ[q] = ((q / Wv + q % Wv + sx + sy) & 1) != 0;  // (the sensor cell stays free)
            if (!show("checkerboard", occ)) return 1;
        }
        if (!show("everything", std::vector<uint8_t>(NC, 1))) return 1;
        // random occupancies with and without walls next to the sensor: the replay alone
        for (int trial = 0; trial < 60; trial++) {
            const double density = trial < 3 ? 0.0 : (trial % 7) * 0.03 + 0.004;
            std::vector<uint8_t> occ(NC, 0);
            for (int q = 0; q < NC; q++) occ[q] = (rng() % 100000) < density * 100000;
            if (trial % 3 == 0) {  // an axis-parallel wall a few cells from the sensor: long left-alone runs, long lists
                const int off = (int)(rng() % 7) - 3;
                if (trial % 2 == 0) {
                    const int a = std::min(std::max(sx + off, 0), Hv - 1);
                    for (int b = 0; b < Wv; b++) occ[a * Wv + b] = 1;
                } else {
                    const int b = std::min(std::max(sy + off, 0), Wv - 1);
                    for (int a = 0; a < Hv; a++) occ[a * Wv + b] = 1;
                }
            }
            if (trial % 4 == 1) occ[sx * Wv + sy] = 0;
            Counts n;
            for (int reset = 0; reset < 2; reset++, n_views++)
                if (!m.run(occ, reset != 0, n, caps, N_CAPS)) return fail(m.why, m.w0, m.w1, m.w2);
        }
    } else if (mode == "file") {
        FILE* fh = fopen(argv[12], "rb");
        if (!fh) return fail("cannot open the views file");
        int32_t head[2];
        if (fread(head, 4, 2, fh) != 2 || head[1] != NC || head[0] < 0) return fail("views file: header", head[0], head[1], NC);
        std::vector<uint8_t> flags(head[0]), occ(NC);
        if (fread(flags.data(), 1, flags.size(), fh) != flags.size()) return fail("views file: flags");
        for (int v = 0; v < head[0]; v++, n_views++) {
            if (fread(occ.data(), 1, NC, fh) != (size_t)NC) return fail("views file: short", v);
            Counts n;
            if (!m.run(occ, flags[v] != 0, n, caps, N_CAPS)) {
                printf("FAIL %s in view %d (%ld %ld %ld)\n", m.why, v, m.w0, m.w1, m.w2);
                return 1;
            }
            printf("V %d %d %d %d %d %d %d %d %d\n", v, n.n_skip, n.flagged, n.passing, n.need_d, n.cap_d, n.need_r, n.cap_r, n.alone_r);
        }
        fclose(fh);
    } else {
        return fail("mode");
    }
    printf("OK %d x %d cells, %d beams: %ld views replayed with the product caps, (5, 2), (0, 0), (any, 2) and (5, any)\n", Hv, Wv, B, n_views);
    return 0;
}
