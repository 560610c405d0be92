// tests/extrema_plan_check.cpp -- prints the launch plan of an extrema pass (3d_sift_cuda_amd/csrc/extrema_plan.h) for the requests
// on its standard input (or, one request, on its command line), one answer per line; built with the host C++ compiler, no HIP.
// tests/test_extrema_plan.py holds the answers against a restatement of the rules.
//   plan X Xl Y Z z_lo z_hi own surv_cap strict pair defer ntaps list2_cap
//        -> plan <status> <form> z0 z1 zchunk z_blocks segments seg_cap tiles_x tiles_y gx gy gz vx vy pair defer lazy_wgs list2_seg_cap
//   seg z_blocks -> seg <segments in use> <segment of z block 0> <of z block 1> ...
//   lazy nx ny nz -> lazy 0|1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "extrema_plan.h"

// the plan is usable in a constant expression: the rows the kernels' comments state
static_assert(extrema_plan_for(512, 512, 512, 512, 0, 512, true, 1 << 20, false, false, false, 0, 0).form == EX_FORM_MARCH, "512^3 marches");
static_assert(extrema_plan_for(512, 512, 512, 512, 0, 512, true, 1 << 20, false, false, false, 0, 0).zchunk == 64, "512^3: chunks of 64");
static_assert(ex_segment_of_z_block(67, 68) == EX_SEGS - 1 && ex_segments_in_use(68) == EX_SEGS, "the last z block takes the last segment");

static int answer(FILE *in)
{
    static const char *const status[] = {"nothing", "ok", "unsupported", "invalid"};
    static const char *const form[] = {"none", "generic", "plane", "march", "strict"};
    char cmd[16];
    while (std::fscanf(in, "%15s", cmd) == 1) {
        if (!std::strcmp(cmd, "plan")) {
            long long X, Xl, Y, Z, surv_cap, list2_cap;
            int z_lo, z_hi, own, strict, pair, defer, ntaps;
            if (std::fscanf(in, "%lld %lld %lld %lld %d %d %d %lld %d %d %d %d %lld", &X, &Xl, &Y, &Z, &z_lo, &z_hi, &own, &surv_cap, &strict, &pair,
                            &defer, &ntaps, &list2_cap) != 13)
                return 2;
            const extrema_plan p = extrema_plan_for(X, Xl, Y, Z, z_lo, z_hi, own != 0, surv_cap, strict != 0, pair != 0, defer != 0, ntaps, list2_cap);
            std::printf("plan %s %s %d %d %d %u %d %lld %d %d %u %u %u %u %u %d %d %u %lld\n", status[p.status], form[p.form], p.z0, p.z1, p.zchunk,
                        p.z_blocks, p.segments, p.seg_cap, p.tiles_x, p.tiles_y, p.grid.x, p.grid.y, p.grid.z, p.vgrid.x, p.vgrid.y, p.pair ? 1 : 0,
                        p.defer ? 1 : 0, p.lazy_wgs, p.list2_seg_cap);
        } else if (!std::strcmp(cmd, "seg")) {
            unsigned n;
            if (std::fscanf(in, "%u", &n) != 1) return 2;
            std::printf("seg %d", ex_segments_in_use(n));
            for (unsigned b = 0; b < n; b++) std::printf(" %d", ex_segment_of_z_block(b, n));
            std::printf("\n");
        } else if (!std::strcmp(cmd, "lazy")) {
            long long nx, ny, nz;
            if (std::fscanf(in, "%lld %lld %lld", &nx, &ny, &nz) != 3) return 2;
            std::printf("lazy %d\n", lazy_shape_ok(nx, ny, nz) ? 1 : 0);
        } else {
            return 2;
        }
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 2) return answer(stdin);
    std::string line;
    for (int i = 1; i < argc; i++) line += std::string(argv[i]) + " ";
    FILE *in = fmemopen(&line[0], line.size(), "r");
    if (!in) return 2;
    const int rc = answer(in);
    std::fclose(in);
    return rc;
}
