// Stand-alone host program over the scalar part of csrc/awr_frame.h -- the crop window and the camera model the prediction path's kernels
// share -- compiled as plain C++ without HIP.  It reads cases from the text file named by argv[1] and prints one line per case: doubles as
// their 64-bit patterns in hex, ints as ints.  tests/test_frame_math_cpu.py builds it with the address and undefined-behaviour sanitizers
// and -ffp-contract=off and compares every figure with the numpy statements (nyu_data.center2bounds, detect._window, detect.palm_center's
// window, evaluator.uvd2xyz / xyz2uvd).
//
// A case is a letter and its doubles (anything strtod reads: hex floats, nan, inf), then its ints:
//   W cu cv cd cube0 cube1 cube2 fx fy fh fw                     -> us ue vs ve | u0 u1 v0 v1 dlo dhi      center_bounds, bounds_window
//   P cu cv cd cube0 cube1 cube2 fx fy search zmin zmax fh fw    -> u0 u1 v0 v1 dlo dhi                    palm_window
//   C u v d fx fy u0 v0 flip                                     -> x y                                    uvd2x, uvd2y
//   X x y z fx fy u0 v0 flip                                     -> u v                                    xyz2u, xyz2v of y * flip
#include <stdio.h>
#include <string.h>

#include "../../awr-adaptive-weighting-regression_amd/csrc/awr_frame.h"

using namespace awr;

static unsigned long long bits(double x) {
    unsigned long long b;
    memcpy(&b, &x, sizeof b);
    return b;
}

static bool read_doubles(FILE* f, double* d, int n) {
    for (int i = 0; i < n; ++i)
        if (fscanf(f, "%lf", d + i) != 1) return false;
    return true;
}

static void print_window(const Window& w) { printf("%d %d %d %d %d %d\n", w.u0, w.u1, w.v0, w.v1, w.dlo, w.dhi); }

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s cases.txt\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    char kind;
    double d[11];
    int fh, fw;
    while (fscanf(f, " %c", &kind) == 1) {
        bool ok = true;
        if (kind == 'W') {
            ok = read_doubles(f, d, 8) && fscanf(f, "%d %d", &fh, &fw) == 2;
            if (ok) {
                const Bounds b = center_bounds(d, d + 3, d[6], d[7]);
                printf("%016llx %016llx %016llx %016llx ", bits(b.us), bits(b.ue), bits(b.vs), bits(b.ve));
                print_window(bounds_window(d, d + 3, d[6], d[7], fh, fw));
            }
        } else if (kind == 'P') {
            ok = read_doubles(f, d, 11) && fscanf(f, "%d %d", &fh, &fw) == 2;
            if (ok) print_window(palm_window(d, d + 3, d[8], d[6], d[7], d[9], d[10], fh, fw));
        } else if (kind == 'C') {
            ok = read_doubles(f, d, 8);
            if (ok) printf("%016llx %016llx\n", bits(uvd2x(d[0], d[5], d[2], d[3])), bits(uvd2y(d[1], d[6], d[2], d[4], d[7])));
        } else if (kind == 'X') {
            ok = read_doubles(f, d, 8);
            if (ok) printf("%016llx %016llx\n", bits(xyz2u(d[0], d[3], d[2], d[5])), bits(xyz2v(d[1] * d[7], d[4], d[2], d[6])));
        } else {
            ok = false;
        }
        if (!ok) { fprintf(stderr, "bad case '%c'\n", kind); fclose(f); return 2; }
    }
    fclose(f);
    return 0;
}
