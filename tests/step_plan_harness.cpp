// Host-only driver of csrc/phd_step_plan.h for tests/test_step_plan.py: reads
// one StepFacts per line from stdin (the fields in declaration order, as
// integers) and prints "<form> <fuse_max>" for each.
#include <cstdio>

#include "phd_step_plan.h"

int main() {
    long v[14];
    for (;;) {
        for (int i = 0; i < 14; i++)
            if (std::scanf("%ld", &v[i]) != 1) return i == 0 ? 0 : 1;
        phd::StepFacts f{};
        f.n = (int)v[0];
        f.n_base = (int)v[1];
        f.n_predict_particles = (int)v[2];
        f.M = (int)v[3];
        f.filter_type = (int)v[4];
        f.feature_model = (int)v[5];
        f.upd_split = (int)v[6];
        f.upd_resident = (int)v[7];
        f.upd_lds = (size_t)v[8];
        f.rs_step_lds = (size_t)v[9];
        f.traced = v[10] != 0;
        f.stamps = v[11] != 0;
        f.overlap_bits = (int)v[12];
        f.lead_on = (int)v[13];
        const phd::StepPlan p = phd::plan_step(f);
        std::printf("%d %d\n", p.form, p.fuse_max ? 1 : 0);
    }
}
