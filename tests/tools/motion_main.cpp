// Runs the live tracker's motion model (host/motion_model.h) on the records of a text file and prints the results, one line a record, every
// number with 17 digits.  Host code only: g++ over this file.
//     motion_main IN
// A record is a line of numbers, the first the operation:
//     0 za[6] zb[6]                                    motion_between           -> wv[6]
//     1 z[6] wv[6]                                     motion_apply             -> out[6]
//     2 frames za[6] zb[6] ta tb time max_dt           motion_measure           -> measured rel[6] pred[6]
//     3 frames za[6] zb[6] ta tb                       motion_velocity          -> vel[6]
//     4 frames za[6] zb[6] ta tb time max_dt           motion_predict           -> pose[6]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../automatic-ar_amd/host/motion_model.h"

using namespace aar;

static void print6(const double *v) {
    for (int k = 0; k < 6; k++) printf(" %.17g", v[k]);
}

static MotionState state(const double *a) {
    MotionState m;
    m.frames = (int)a[0];
    for (int k = 0; k < 6; k++) { m.za[k] = a[1 + k]; m.zb[k] = a[7 + k]; }
    m.ta = a[13]; m.tb = a[14];
    return m;
}

int main(int argc, char **argv) {
    if (argc < 2) { fputs("usage: motion_main IN\n", stderr); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    static const int need[5] = {12, 12, 17, 15, 17};
    int op;
    while (fscanf(f, "%d", &op) == 1) {
        if (op < 0 || op > 4) { fprintf(stderr, "bad operation %d\n", op); return 2; }
        std::vector<double> a(need[op]);
        for (double &v : a)
            if (fscanf(f, "%lf", &v) != 1) { fputs("short record\n", stderr); return 2; }
        double out[6], rel[6];
        if (op == 0) {
            motion_between(a.data(), a.data() + 6, out);
            print6(out);
        } else if (op == 1) {
            motion_apply(a.data(), a.data() + 6, out);
            print6(out);
        } else if (op == 2) {
            const bool measured = motion_measure(state(a.data()), a[15], a[16], rel, out);
            printf(" %d", measured ? 1 : 0);
            print6(rel);
            print6(out);
        } else if (op == 3) {
            motion_velocity(state(a.data()), out);
            print6(out);
        } else {
            motion_predict(state(a.data()), a[15], a[16], out);
            print6(out);
        }
        printf("\n");
    }
    fclose(f);
    return 0;
}
