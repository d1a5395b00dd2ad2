// Host driver of ray_root (pylabfea_amd/csrc/plfx_rayroot.hpp) for tests/test_rayroot_cpu.py: the search on scalar functions
// whose values are single IEEE operations, so that this program, the test's Python transcription and the device agree bit
// for bit.  stdin: one case per line, "id a b c x0" (numbers as strtod reads them, hex floats included); stdout per case:
// the root as a hex float, the status, the number of evaluations of f.
//   0  x - a                              1  a - x (the wrong sign convention)
//   2  b for x >= a, else -b (a step)     3  a (constant; a may be NaN)
//   4  x - c, but NaN where x > a (b > 0) or x < a (b < 0)
//   5  x - a until both signs have been seen, then +1, -1, +1, ... whatever x is
#include <cstdio>
#include <cstdlib>

#include "plfx_rayroot.hpp"

int main()
{
    char line[512];
    while (fgets(line, sizeof line, stdin)) {
        char *p = line;
        const int id = (int)strtol(p, &p, 10);
        double v[4];
        for (int k = 0; k < 4; k++) {
            char *q;
            v[k] = strtod(p, &q);
            if (q == p) {
                fprintf(stderr, "bad case: %s", line);
                return 2;
            }
            p = q;
        }
        const double a = v[0], b = v[1], c = v[2], x0 = v[3], nan = __builtin_nan("");
        long evals = 0;
        bool neg = false, pos = false, up = false;
        double root = 0.;
        const int st = plfx::ray_root(
            x0,
            [&](double x) -> double {
                evals++;
                switch (id) {
                case 0: return x - a;
                case 1: return a - x;
                case 2: return x >= a ? b : -b;
                case 3: return a;
                case 4: return ((b > 0. && x > a) || (b < 0. && x < a)) ? nan : x - c;
                case 5:
                    if (neg && pos) return (up = !up) ? 1. : -1.;
                    (x - a < 0. ? neg : pos) = true;
                    return x - a;
                }
                return nan;
            },
            root);
        if (root != root)
            printf("nan %d %ld\n", st, evals);
        else
            printf("%a %d %ld\n", root, st, evals);
    }
    return 0;
}
