// Stand-alone driver of csrc/scalar_log.h for tests/test_scalar_log_cpu.py: reads n and n doubles, writes scalar_log of each.
#include "scalar_log.h"
#include <cstdio>
#include <vector>

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    int64_t n = 0;
    if (std::fread(&n, sizeof(n), 1, f) != 1 || n < 0) return 4;
    std::vector<double> x((size_t)n), y((size_t)n);
    if (std::fread(x.data(), sizeof(double), (size_t)n, f) != (size_t)n) return 5;
    std::fclose(f);
    for (int64_t i = 0; i < n; ++i) y[(size_t)i] = mih::scalar_log(x[(size_t)i]);
    f = std::fopen(argv[2], "wb");
    if (!f) return 6;
    if (std::fwrite(y.data(), sizeof(double), (size_t)n, f) != (size_t)n) return 7;
    std::fclose(f);
    return 0;
}
