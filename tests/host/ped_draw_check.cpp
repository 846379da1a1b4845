// ped_draw_check.cpp -- the per-item functions of img_env_amd/csrc/ped_draw.h on the CPU, over a simulated grid.
//   g++ -std=c++17 -ffp-contract=off tests/host/ped_draw_check.cpp -o check && ./check case.bin result.bin
// (also built with -fsanitize=address,undefined by tests/test_ped_draw_model.py)
//
// The case file (little endian): int32 PV, Hp, Wp, m, n, mode, first, TR, grid, wide, n_index; float64 res, inv_res, r, r2;
// float32 vectors[m][PV]; int32 index[n_index].  mode 0: row i from vector i; 1: from index[i] (`rows`); 2: from index[first + i]
// where first + i < TR (the minibatch's `order`).  The result file: float32 out[n][3][Hp][Wp], filled with a pattern first so that
// a cell nobody wrote shows.  The walk below is k_ped_draw's: workgroups stride over the rows, lanes over the plane, the
// pedestrians and the cells; what the barriers separate runs phase after phase, the LDS atomicMax is a max.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../img_env_amd/csrc/ped_draw.h"

static bool read_all(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
    if (argc != 3) return printf("usage: %s case.bin result.bin\n", argv[0]), 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return printf("cannot open %s\n", argv[1]), 2;
    int32_t hd[11];
    double geo[4];
    if (!read_all(f, hd, sizeof(hd)) || !read_all(f, geo, sizeof(geo))) return printf("short header\n"), 2;
    const int PV = hd[0], Hp = hd[1], Wp = hd[2], m = hd[3], n = hd[4], mode = hd[5], first = hd[6], TR = hd[7], grid = hd[8], wide = hd[9], n_index = hd[10];
    if (PV < 1 || m < 0 || n < 0 || grid < 1 || n_index < 0 || !plan_ped_draw_fits(Hp, Wp)) return printf("bad case\n"), 2;
    std::vector<float> vec((size_t)m * PV + 1);
    std::vector<int32_t> index((size_t)n_index + 1);
    if (!read_all(f, vec.data(), (size_t)m * PV * 4) || !read_all(f, index.data(), (size_t)n_index * 4)) return printf("short case\n"), 2;
    fclose(f);
    const size_t NP = (size_t)Hp * Wp;
    if (wide && NP % 4) return printf("bad case: wide\n"), 2;
    std::vector<FieldChunk16> out_store(((size_t)n * 3 * NP + 3) / 4 + 1);  // (16-byte aligned, as the wide stores need)
    uint32_t* out = (uint32_t*)out_store.data();
    for (size_t k = 0; k < (size_t)n * 3 * NP; k++) out[k] = 0x7fc0dead;

    PedDrawDev d = {};
    d.vec = vec.data();
    d.out = (float*)out;
    d.rows = mode == 1 ? index.data() : nullptr;
    d.order = mode == 2 ? index.data() : nullptr;
    d.first = (size_t)first;
    d.TR = (uint32_t)TR;
    d.n = (uint32_t)n;
    d.PV = PV; d.Hp = Hp; d.Wp = Wp;
    d.wide = wide;
    d.res = geo[0]; d.inv_res = geo[1]; d.r = geo[2]; d.r2 = geo[3];

    const LaunchShape shape = plan_ped_draw_launch((size_t)n, Hp, Wp);
    if (shape.block != PED_DRAW_BLOCK || shape.lds != NP * 4 || shape.grid < 1 || shape.grid > PED_DRAW_MAX_BLOCKS) return printf("bad launch shape\n"), 1;
    std::vector<FieldChunk16> plane_store(NP / 4 + 1);
    uint32_t* plane = (uint32_t*)plane_store.data();
    size_t stamped = 0;
    for (int block = 0; block < grid; block++)
        for (size_t i = (size_t)block; i < (size_t)n; i += (size_t)grid) {
            const int64_t src = ped_draw_src(d, i);
            if (src >= m) return printf("bad case: source row %lld of %d\n", (long long)src, m), 2;
            const float* v = d.vec + (size_t)(src < 0 ? 0 : src) * (size_t)PV;
            const int n_ped = src < 0 ? 0 : ped_draw_count(v, PV);
            uint32_t* o = out + i * 3 * NP;
            if (n_ped > 0) {
                for (uint32_t tid = 0; tid < PED_DRAW_BLOCK; tid++)
                    for (size_t c = tid; c < NP; c += PED_DRAW_BLOCK) plane[c] = 0u;
                for (uint32_t tid = 0; tid < PED_DRAW_BLOCK; tid++)
                    for (int q = (int)tid; q < n_ped; q += PED_DRAW_BLOCK)
                        ped_draw_stamp(d, v, q, [&](int c, uint32_t rank) {
                            if (c < 0 || (size_t)c >= NP) exit((printf("cell %d outside the plane\n", c), 1));
                            plane[c] = std::max(plane[c], rank);
                            stamped++;
                        });
            }
            for (uint32_t tid = 0; tid < PED_DRAW_BLOCK; tid++) {
                if (wide) {
                    const FieldChunk16 zero = {};
                    for (size_t c = tid; c < NP / 4; c += PED_DRAW_BLOCK) ped_draw_store4((const uint32_t*)v, n_ped > 0 ? plane_store[c] : zero, o, NP, c);
                } else {
                    for (size_t c = tid; c < NP; c += PED_DRAW_BLOCK) ped_draw_store1((const uint32_t*)v, n_ped > 0 ? plane[c] : 0u, o, NP, c);
                }
            }
        }
    FILE* g = fopen(argv[2], "wb");
    if (!g || fwrite(out, 4, (size_t)n * 3 * NP, g) != (size_t)n * 3 * NP) return printf("cannot write %s\n", argv[2]), 2;
    fclose(g);
    printf("OK %zu\n", stamped);
    return 0;
}
