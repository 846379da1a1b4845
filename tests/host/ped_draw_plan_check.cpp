// ped_draw_plan_check.cpp -- what the enable calls decide about IMGENV_ROLLOUT_PED_MAPS_DRAWN before they touch a device
// (img_env_amd/csrc/feature_plan.h, the slot catalogue of obs_fields.h, the launch shape of launch_plan.h), on the CPU.
//   g++ -std=c++17 tests/host/ped_draw_plan_check.cpp -o check && ./check
// (also built with -fsanitize=address,undefined by tests/test_ped_draw_abi.py)
#include <string>

#include "../../img_env_amd/csrc/feature_plan.h"

static int n_bad = 0, n_checks = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        n_checks++;                                                  \
        if (!(cond)) {                                               \
            n_bad++;                                                 \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                            \
    } while (0)
#define REFUSED(call, code, text)                                           \
    do {                                                                    \
        FeatureMsg msg = "";                                                \
        const int rc_ = (call);                                             \
        CHECK(rc_ == (code));                                               \
        CHECK(std::string(msg) == (text));                                  \
        if (std::string(msg) != (text)) printf("  got %d: %s\n", rc_, msg); \
    } while (0)
#define ACCEPTED(call, code) REFUSED(call, code, "")

enum { SM = IMGENV_ROLLOUT_SENSOR_MAPS, VS = IMGENV_ROLLOUT_VECTOR_STATES, PV = IMGENV_ROLLOUT_PED_VECTOR_STATES, PM = IMGENV_ROLLOUT_PED_MAPS,
       DRAWN = IMGENV_ROLLOUT_PED_MAPS_DRAWN };

static FeatureFacts handle(int ped_h, int ped_w) {
    FeatureFacts f;
    f.RL = 4; f.P = 3; f.state_dim = 3; f.ped_vec_dim = 7; f.n_beams = 181;
    f.keep_view_maps = true;
    f.ped_h = ped_h; f.ped_w = ped_w;
    return f;
}
static const void* fake(int k) { return (const void*)(uintptr_t)(4096 * (k + 1)); }
// the catalogue of a handle with 48 x 48 pedestrian maps and ped_vec_len 71, no optional array
static void catalogue(ObsField (&f)[OBSF_COUNT]) {
    ObsFacts a;
    memset(&a, 0, sizeof(a));
    a.out.view_h = a.out.view_w = a.out.image_h = a.out.image_w = 48;
    a.out.n_beams = 181; a.out.state_dim = 3; a.out.ped_vec_len = 71;
    a.ped_image_size[0] = a.ped_image_size[1] = 48;
    a.out.vector_states = (float*)fake(0); a.out.sensor_maps = (uint16_t*)fake(1); a.out.lasers = (double*)fake(2);
    a.out.ped_vector_states = (float*)fake(3); a.out.ped_maps = (float*)fake(4);
    obs_fields(a, f);
}

int main() {
    CHECK(IMGENV_ROLLOUT_PED_MAPS_DRAWN == 512 && IMGENV_ROLLOUT_ALL == 127 && !(IMGENV_ROLLOUT_ALL & DRAWN));
    CHECK(!(DRAWN & (IMGENV_ROLLOUT_NORM_STATES | IMGENV_ROLLOUT_NORM_REWARDS)));

    // ---- imgenv_rollout_enable
    FeatureFacts f = handle(48, 48);
    imgenv_rollout_cfg c = {};
    c.struct_size = (int32_t)sizeof(c); c.horizon = 3; c.final_capacity = 4;
    c.fields = SM | PV | DRAWN;
    ACCEPTED(rollout_enable_plan(&c, nullptr, &f, nullptr, msg), IMGENV_OK);
    c.fields = PV | DRAWN;
    ACCEPTED(rollout_enable_plan(&c, nullptr, &f, nullptr, msg), IMGENV_OK);
    // the two illegal combinations, in front of the null handle like every refusal of the cfg alone
    c.fields = SM | PV | PM | DRAWN;
    REFUSED(rollout_enable_plan(&c, nullptr, &f, nullptr, msg), IMGENV_EINVAL, "imgenv_rollout_cfg.fields 537: IMGENV_ROLLOUT_PED_MAPS_DRAWN excludes IMGENV_ROLLOUT_PED_MAPS");
    REFUSED(rollout_enable_plan(&c, nullptr, nullptr, nullptr, msg), IMGENV_EINVAL, "imgenv_rollout_cfg.fields 537: IMGENV_ROLLOUT_PED_MAPS_DRAWN excludes IMGENV_ROLLOUT_PED_MAPS");
    c.fields = SM | DRAWN;
    REFUSED(rollout_enable_plan(&c, nullptr, &f, nullptr, msg), IMGENV_EINVAL, "imgenv_rollout_cfg.fields 513: IMGENV_ROLLOUT_PED_MAPS_DRAWN needs IMGENV_ROLLOUT_PED_VECTOR_STATES");
    REFUSED(rollout_enable_plan(&c, nullptr, nullptr, nullptr, msg), IMGENV_EINVAL, "imgenv_rollout_cfg.fields 513: IMGENV_ROLLOUT_PED_MAPS_DRAWN needs IMGENV_ROLLOUT_PED_VECTOR_STATES");
    c.fields = PM | DRAWN;  // (both at once: the missing vector is named first)
    REFUSED(rollout_enable_plan(&c, nullptr, &f, nullptr, msg), IMGENV_EINVAL, "imgenv_rollout_cfg.fields 528: IMGENV_ROLLOUT_PED_MAPS_DRAWN needs IMGENV_ROLLOUT_PED_VECTOR_STATES");
    c.fields = DRAWN;
    REFUSED(rollout_enable_plan(&c, nullptr, &f, nullptr, msg), IMGENV_EINVAL, "imgenv_rollout_cfg.fields 512");
    c.fields = 1024 | PV;
    REFUSED(rollout_enable_plan(&c, nullptr, &f, nullptr, msg), IMGENV_EINVAL, "imgenv_rollout_cfg.fields 1032");
    // the rank plane: 96 x 96 and 128 x 128 fit, 129 x 128 does not
    c.fields = PV | DRAWN;
    f = handle(96, 96);
    ACCEPTED(rollout_enable_plan(&c, nullptr, &f, nullptr, msg), IMGENV_OK);
    f = handle(128, 128);
    ACCEPTED(rollout_enable_plan(&c, nullptr, &f, nullptr, msg), IMGENV_OK);
    f = handle(129, 128);
    REFUSED(rollout_enable_plan(&c, nullptr, &f, nullptr, msg), IMGENV_EINVAL,
            "imgenv_rollout_cfg.fields 520: IMGENV_ROLLOUT_PED_MAPS_DRAWN with pedestrian maps of 129 x 128 cells (a plane of 65536 bytes at most)");
    c.fields = PV | PM;  // (a ring that stores its maps takes any geometry)
    ACCEPTED(rollout_enable_plan(&c, nullptr, &f, nullptr, msg), IMGENV_OK);
    CHECK(plan_ped_draw_fits(96, 96) && plan_ped_draw_fits(128, 128) && !plan_ped_draw_fits(129, 128) && !plan_ped_draw_fits(0, 48) && !plan_ped_draw_fits(48, -1));
    CHECK(plan_ped_draw_lds(96, 96) == 36864);
    const LaunchShape one = plan_ped_draw_launch(1, 48, 48), many = plan_ped_draw_launch(100000, 40, 40);
    CHECK(one.grid == 1 && one.block == PED_DRAW_BLOCK && one.lds == 9216);
    CHECK(many.grid == PED_DRAW_MAX_BLOCKS && many.block == PED_DRAW_BLOCK && many.lds == 6400);
    // the repeated call compares the bit like any other
    f = handle(48, 48);
    f.roll_on = true;
    imgenv_rollout_cfg stored = c;
    stored.fields = SM | PV | DRAWN;
    c.fields = SM | PV | DRAWN;
    ACCEPTED(rollout_enable_plan(&c, nullptr, &f, &stored, msg), ENABLE_REPEAT);
    c.fields = SM | PV;
    REFUSED(rollout_enable_plan(&c, nullptr, &f, &stored, msg), IMGENV_EINVAL, "imgenv_rollout_enable: the handle already keeps a rollout of horizon 3, final_capacity 4, fields 521");

    // ---- imgenv_rollout_minibatch_enable
    f = handle(48, 48);
    f.roll_on = true; f.roll_horizon = 3; f.roll_fields = SM | PV | DRAWN;
    imgenv_minibatch_cfg m = {};
    m.struct_size = (int32_t)sizeof(m); m.batch = 4; m.buffers = 2; m.fields = 0;
    int want = -1;
    ACCEPTED(minibatch_enable_plan(&m, nullptr, &f, nullptr, &want, msg), IMGENV_OK);
    CHECK(want == (SM | PV | DRAWN));  // 0: every field of the rollout, the drawn one too
    m.fields = DRAWN;
    ACCEPTED(minibatch_enable_plan(&m, nullptr, &f, nullptr, &want, msg), IMGENV_OK);
    CHECK(want == DRAWN);  // (the minibatch needs the vector only if the caller selects it)
    m.fields = PM;
    REFUSED(minibatch_enable_plan(&m, nullptr, &f, nullptr, &want, msg), IMGENV_EINVAL, "imgenv_minibatch_cfg.fields 16: the rollout stores 521");
    f.roll_fields = SM | PV | PM;
    m.fields = DRAWN;
    REFUSED(minibatch_enable_plan(&m, nullptr, &f, nullptr, &want, msg), IMGENV_EINVAL, "imgenv_minibatch_cfg.fields 512: the rollout stores 25");
    m.fields = 1024;
    REFUSED(minibatch_enable_plan(&m, nullptr, &f, nullptr, &want, msg), IMGENV_EINVAL, "imgenv_minibatch_cfg.fields 1024");

    // ---- the slot table: a minibatch slot, no ring slot, no final slot
    const ObsSlot& slot = OBS_SLOTS[OBSF_PED_MAPS_DRAWN];
    CHECK(slot.final_bit == 0 && slot.rollout_bit == DRAWN && !slot.norm);
    CHECK(slot.final_out == OBS_NO_SLOT && slot.ring_out == OBS_NO_SLOT && slot.fin_out == OBS_NO_SLOT);
    CHECK(slot.mb_out == offsetof(imgenv_minibatch_buffer, mb_ped_maps) && slot.mb_out == OBS_SLOTS[OBSF_PED_MAPS].mb_out);
    CHECK(slot.from == OBSF_PED_VECTOR_STATES);
    CHECK(OBSF_PED_MAPS_DRAWN == OBSF_COUNT && OBSF_SLOT_COUNT == OBSF_COUNT + 1);  // (behind the fields a handle has arrays of)
    for (int k = 0; k < OBSF_COUNT; k++) CHECK(OBS_SLOTS[k].from == -1);
    for (int which = FIELDS_FINAL; which <= FIELDS_ROLLOUT; which++) {  // no order but the minibatches' lists it
        const FieldFeatureNames n = field_feature((FieldFeature)which);
        for (int k = 0; k < n.n_order; k++) CHECK(n.order[k] != OBSF_PED_MAPS_DRAWN);
    }
    ObsField cat[OBSF_COUNT];
    catalogue(cat);
    const size_t map_row = ped_maps_row_bytes(handle(48, 48));
    CHECK(map_row == 27648 && ped_maps_row_bytes(handle(40, 96)) == 46080 && ped_maps_row_bytes(handle(0, 0)) == 0);
    {   // with the drawn fields behind it: from the vectors' array, with the row the caller names
        ObsField ext[OBSF_SLOT_COUNT];
        obs_fields_with_drawn(cat, map_row, ext);
        CHECK(ext[OBSF_PED_MAPS_DRAWN].src == cat[OBSF_PED_VECTOR_STATES].src && ext[OBSF_PED_MAPS_DRAWN].row_bytes == 27648);
        for (int k = 0; k < OBSF_COUNT; k++) CHECK(ext[k].src == cat[k].src && ext[k].row_bytes == cat[k].row_bytes);
    }
    FieldSelection s;
    {   // the ring of (sensor_maps, ped_vector_states, drawn): two fields, none of them the drawn one
        ACCEPTED(select_feature_fields(FIELDS_ROLLOUT, cat, SM | PV | DRAWN, SM | PV | DRAWN, s, msg), IMGENV_OK);
        CHECK(s.n == 2 && s.id[0] == OBSF_SENSOR_MAPS && s.id[1] == OBSF_PED_VECTOR_STATES && s.row_bytes[1] == 284);
        const int five = IMGENV_FINAL_VECTOR_STATES | IMGENV_FINAL_SENSOR_MAPS | IMGENV_FINAL_LASERS | IMGENV_FINAL_PED_VECTOR_STATES | IMGENV_FINAL_PED_MAPS;
        ACCEPTED(select_feature_fields(FIELDS_FINAL, cat, five, five, s, msg), IMGENV_OK);
        CHECK(s.n == 5);
        for (int k = 0; k < s.n; k++) CHECK(s.id[k] != OBSF_PED_MAPS_DRAWN);
    }
    {   // what that ring keeps, as imgenv_rollout_minibatch_enable lays it out: no ring of maps; the drawn row's length comes with the call
        ObsField ring[OBSF_COUNT] = {};
        ring[OBSF_SENSOR_MAPS] = {fake(20), 4608};
        ring[OBSF_PED_VECTOR_STATES] = {fake(21), 284};
        REFUSED(select_feature_fields(FIELDS_MINIBATCH, ring, DRAWN, DRAWN, s, msg), IMGENV_EINVAL,
                "imgenv_minibatch_cfg.fields: bit 512 names a field of no bytes on this handle");  // (no length given)
        ACCEPTED(select_feature_fields(FIELDS_MINIBATCH, ring, SM | PV | DRAWN, 0, s, msg, map_row), IMGENV_OK);
        CHECK(s.n == 3 && s.id[0] == OBSF_SENSOR_MAPS && s.id[1] == OBSF_PED_VECTOR_STATES && s.id[2] == OBSF_PED_MAPS_DRAWN);
        CHECK(s.row_bytes[2] == 27648);
        ACCEPTED(select_feature_fields(FIELDS_MINIBATCH, ring, DRAWN, DRAWN, s, msg, map_row), IMGENV_OK);
        CHECK(s.n == 1 && s.id[0] == OBSF_PED_MAPS_DRAWN);  // ONE minibatch slot, without the vector
        imgenv_minibatch_buffer mb = {};
        imgenv_normalise_out no = {};
        obs_slot_put_mb(OBS_SLOTS[s.id[0]], &mb, &no, 1, (void*)fake(30));
        CHECK(mb.mb_ped_maps == (float*)fake(30) && mb.mb_ped_vector_states == nullptr);
        // a ring without the vectors has no source for it: the field is skipped like any optional one the handle lacks
        ring[OBSF_PED_VECTOR_STATES] = {};
        REFUSED(select_feature_fields(FIELDS_MINIBATCH, ring, DRAWN, DRAWN, s, msg, map_row), IMGENV_EINVAL, "imgenv_minibatch_cfg.fields 512: no field of the rollout");
    }
    if (n_bad) return printf("%d of %d checks failed\n", n_bad, n_checks), 1;
    printf("OK %d\n", n_checks);
    return 0;
}
