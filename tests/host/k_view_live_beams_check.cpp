// CPU check of k_view's first hits over live beams only (one wavefront, img_env_amd/csrc/kernels.h phase 3), without a GPU:
// the kernel's walk -- chunk 0 of every beam in rounds of 64 lanes, then chunk ch + 1 only of the beams that neither hit nor
// ended in chunk ch, taken 64 at a time from a queue of beam numbers compacted in place -- restated on the host with the
// library's own tables (host_tables.h build_robot_class) and compared with each beam's first occupied cell on its path, on
// random crops (occupied 0, free 255, out of the map 200) with and without axis-parallel walls and with hits placed on the
// last / first step of a chunk.  Also prints how many 64-lane chunk walks the old walk (every round until its last beam is
// done) and the live-beam walk take.
// usage: k_view_live_beams_check <view_w> <view_h> <res> <beams> <angle_begin> <angle_end> <seed> [tables] ; exit code 0 = all good
#include <stdio.h>

#include <random>

#define WAVE_SZ 64
#include "../../img_env_amd/csrc/host_tables.h"

static int fail(const char* what, long a = 0, long b = 0, long c = 0) {
    printf("FAIL %s (%ld %ld %ld)\n", what, a, b, c);
    return 1;
}

int main(int argc, char** argv) {
    if (argc < 8) return fail("usage");
    imgenv_cfg c;
    memset(&c, 0, sizeof(c));
    c.view_width = (float)atof(argv[1]);
    c.view_height = (float)atof(argv[2]);
    c.view_resolution = (float)atof(argv[3]);
    c.use_laser = 1;
    c.range_total = atoi(argv[4]);
    c.view_angle_begin = (float)atof(argv[5]);
    c.view_angle_end = (float)atof(argv[6]);
    c.view_min_dist = -100.f;
    c.view_max_dist = 100.f;
    const unsigned seed = (unsigned)atoi(argv[7]);
    const ViewGeom g = make_view_geom(c);
    RobotClassHost k;
    k.shape = IMGENV_SHAPE_CIRCLE;
    k.size[0] = 0.f; k.size[1] = 0.f; k.size[2] = 0.17f; k.size[3] = 0.f;
    k.sensor[0] = 0.f; k.sensor[1] = 0.f;
    build_robot_class(k, g);
    if (!k.ok) return fail("class tables overflow");
    if (k.big) { printf("SKIP big class\n"); return 0; }
    const int Hv = g.Hv, Wv = g.Wv, NC = Hv * Wv, B = g.B, S = k.ray_stride, n_chunks = k.ray_kpad / 8;
    if (B > 8 * Wv) { printf("OK the queue does not fit the column table: the kernel keeps the old walk\n"); return 0; }
    if (n_chunks < 1 || k.ray_kpad % 8 != 0) return fail("ray_kpad", k.ray_kpad);
    for (int b = 0; b < B; b++)
        if (k.ray_len[b] > k.ray_kpad) return fail("a beam longer than its padded chunks", b, k.ray_len[b]);
    if (argc > 8 && !strcmp(argv[8], "tables")) {  // for tools/beam_work.py: each beam's length and hit distance per step
        printf("%d %d\n", B, n_chunks);
        for (int b = 0; b < B; b++) {
            printf("%d", (int)k.ray_len[b]);
            for (int q = 0; q < k.ray_len[b]; q++) printf(" %.9g", (double)k.ray_dist[(size_t)q * S + b]);
            printf("\n");
        }
        return 0;
    }
    auto cell_of = [&](int b, int q) { return (int)k.ray_rows[((q / 8) * (size_t)S + b) * 8 + (q % 8)]; };
    // one chunk of one beam, as beam_chunk_key: min over its 8 steps of value << 8 | step
    auto chunk_key = [&](const std::vector<uint8_t>& src, int b, int ch) {
        uint32_t key = 0xFFFFFFFFu;
        for (int j = 0; j < 8; j++) key = std::min(key, ((uint32_t)src[cell_of(b, 8 * ch + j)] << 8) | (uint32_t)(8 * ch + j));
        return key;
    };
    std::mt19937 rng(seed);
    long walks_old = 0, walks_new = 0;
    for (int trial = 0; trial < 60; trial++) {
        const double density = trial < 4 ? 0.0 : (trial % 5) * 0.02 + 0.004;
        std::vector<uint8_t> src(NC + 16, 255);  // + the free dummy cells padded path entries point at
        for (int q = 0; q < NC; q++) {
            const uint32_t r = rng() % 100000;
            src[q] = r < density * 100000 ? 0 : (r > 97000 && trial % 2 ? 200 : 255);
        }
        if (trial % 3 == 0)  // an axis-parallel wall
            for (int y = 0; y < Wv; y++) src[(rng() % Hv) * Wv + y] = 0;
        if (trial % 4 == 1)  // hits on chunk boundaries: the last step of a chunk or the first of the next
            for (int b = 0; b < B; b += 3) {
                const int q = 8 * (1 + (int)(rng() % 3)) - (int)(rng() % 2);
                if (q < k.ray_len[b]) src[cell_of(b, q)] = 0;
            }
        // reference: each beam's first occupied cell
        std::vector<int> hk(B, -1);
        for (int b = 0; b < B; b++)
            for (int q = 0; q < k.ray_len[b]; q++)
                if (src[cell_of(b, q)] == 0) { hk[b] = q; break; }
        // old walk: per round of 64 beams, chunks until every lane has hit or ended
        for (int b0 = 0; b0 < B; b0 += 64) {
            int need = 1;
            for (int b = b0; b < std::min(b0 + 64, B); b++) need = std::max(need, hk[b] >= 0 ? hk[b] / 8 + 1 : std::max(1, (k.ray_len[b] + 7) / 8));
            walks_old += std::min(need, n_chunks);
        }
        // the live-beam walk
        std::vector<uint32_t> hit(B, 0xDEADBEEFu);
        std::vector<uint16_t> queue(B);
        int n_live = 0;
        for (int b0 = 0; b0 < B; b0 += 64) {
            walks_new++;
            std::vector<int> surv;
            for (int b = b0; b < std::min(b0 + 64, B); b++) {
                const uint32_t first = chunk_key(src, b, 0);
                const bool live = first >= 0x0100u && k.ray_len[b] > 8;
                if (!live) hit[b] = first;
                else surv.push_back(b);
            }
            for (int s : surv) queue[n_live++] = (uint16_t)s;
        }
        for (int ch = 1; ch < n_chunks && n_live > 0; ch++) {
            int n_next = 0;
            for (int q0 = 0; q0 < n_live; q0 += 64) {
                walks_new++;
                std::vector<int> got;  // a round reads its entries before it writes its survivors
                for (int j = q0; j < std::min(q0 + 64, n_live); j++) got.push_back(queue[j]);
                std::vector<int> surv;
                for (int b : got) {
                    const uint32_t first = chunk_key(src, b, ch);
                    const bool live = first >= 0x0100u && k.ray_len[b] > 8 * ch + 8;
                    if (!live) hit[b] = first;
                    else surv.push_back(b);
                }
                if (n_next + (int)surv.size() > q0 + (int)got.size()) return fail("survivors overtake the unread entries", ch, q0);
                for (int s : surv) queue[n_next++] = (uint16_t)s;
            }
            n_live = n_next;
        }
        if (n_live != 0) return fail("beams alive behind the last chunk", n_live);
        for (int b = 0; b < B; b++) {
            if (hit[b] == 0xDEADBEEFu) return fail("a beam without a key", trial, b);
            const bool has = hit[b] < 0x0100u;
            if (has != (hk[b] >= 0) || (has && (int)(hit[b] & 0xFFu) != hk[b])) return fail("first hit", trial, b, hk[b]);
        }
    }
    printf("OK %d beams, %d chunks: 64-lane chunk walks %ld (every round to its last beam) -> %ld (live beams)\n", B, n_chunks, walks_old,
           walks_new);
    return 0;
}
