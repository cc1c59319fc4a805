// Stand-alone harness of csrc/normal_tail.h: reads z values (one per line) from standard input and prints -log10 p of each with
// 17 significant digits.  Built by tests/test_normal_tail_cpu.py with g++, plainly and under the address and undefined-behaviour
// sanitizers.
#include <cstdio>
#include <vector>

#include "normal_tail.h"

int main()
{
    std::vector<double> z;
    double v;
    while (std::scanf("%lf", &v) == 1) z.push_back(v);
    for (double x : z) std::printf("%.17g\n", mih::neglog10p_of_z(x));
    return 0;
}
