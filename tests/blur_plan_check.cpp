// tests/blur_plan_check.cpp -- prints the launch plan of the fused blur (3d_sift_cuda_amd/csrc/blur_plan.h) for the requests on
// its standard input, one answer per line; built with the host C++ compiler, no HIP.  tests/test_blur_plan.py holds the answers
// against a restatement of the rules.
//   plan R out dog X Y Z zo0 zo1 sub chunks rows tile order stagger resident
//        -> plan <form> zlen nch tiles_x tiles_y total order   (or: plan <form> outside)
//   fuse mode ntaps X Y Z -> fuse 0|1        inside ntaps X Y -> inside 0|1
//   forms -> form <form>, one line per form the kernel table holds
#include <cstdio>
#include <cstring>

#include "blur_plan.h"

static void print_form(const char *what, const blur_form &f)
{
    const auto b = [](bool v) { return v ? "true" : "false"; };
    std::printf("%s <%d,%d,%s,%s,%d,%d,%d,%s,%s>", what, f.R, f.rows, b(f.has_out), b(f.has_dog), f.pf, f.tx, f.ty, b(f.has_sub), b(f.stg));
}

int main()
{
    char cmd[16];
    while (std::scanf("%15s", cmd) == 1) {
        if (!std::strcmp(cmd, "plan")) {
            int R, out, dog, sub, resident;
            long long X, Y, Z, zo0, zo1;
            sift3d_blur_tuning k;
            if (std::scanf("%d %d %d %lld %lld %lld %lld %lld %d %d %d %d %d %d %d", &R, &out, &dog, &X, &Y, &Z, &zo0, &zo1, &sub, &k.z_chunks,
                           &k.rows_per_thread, &k.tile, &k.order, &k.stagger, &resident) != 15)
                return 2;
            const blur_form f = blur_choose_form(R, out != 0, dog != 0, X, Y, Z, zo0, zo1, sub != 0, k);
            blur_chunking c;
            print_form("plan", f);
            if (blur_plan_chunks(f, X, Y, zo0, zo1, resident, k, &c)) std::printf(" %d %d %d %d %lld %d\n", c.zlen, c.nch, c.tiles_x, c.tiles_y, c.total, c.order);
            else std::printf(" outside\n");
        } else if (!std::strcmp(cmd, "fuse")) {
            int mode, ntaps;
            long long X, Y, Z;
            if (std::scanf("%d %d %lld %lld %lld", &mode, &ntaps, &X, &Y, &Z) != 5) return 2;
            std::printf("fuse %d\n", blur_takes_fused(mode, ntaps, (double)X * Y * Z) ? 1 : 0);
        } else if (!std::strcmp(cmd, "inside")) {
            int ntaps;
            long long X, Y;
            if (std::scanf("%d %lld %lld", &ntaps, &X, &Y) != 3) return 2;
            std::printf("inside %d\n", blur_shape_inside(ntaps, X, Y) ? 1 : 0);
        } else if (!std::strcmp(cmd, "forms")) {
            for (int i = 0; i < BLUR_FORM_CANDIDATES; i++)
                if (blur_form_exists(blur_form_candidate(i))) {
                    print_form("form", blur_form_candidate(i));
                    std::printf("\n");
                }
        } else {
            return 2;
        }
    }
    return 0;
}
