// Stand-alone driver of csrc/sym_eig.h for tests/test_sym_eig_cpu.py: plain C++, no HIP, no library.
//   sym_eig_harness eig  in out    in: int64 n, n * n doubles (row-major)    out: n doubles w, n * n doubles V, 1 double sweeps
//   sym_eig_harness rank in out    in: int64 n, n doubles (descending)       out: 1 double, the surviving directions
//   sym_eig_harness sign in out    in: int64 n, n doubles                    out: n doubles with the sign rule applied
#include <cstdio>
#include <cstring>
#include <vector>

#include "sym_eig.h"

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: %s eig|rank|sign in out\n", argv[0]); return 2; }
    FILE *f = fopen(argv[2], "rb");
    if (!f) { perror(argv[2]); return 2; }
    int64_t n = 0;
    if (fread(&n, sizeof(n), 1, f) != 1 || n < 0 || n > (1 << 20)) { fprintf(stderr, "bad header\n"); return 2; }
    const bool eig = !strcmp(argv[1], "eig");
    if (eig && n > mih::kSymEigMaxOrder) { fprintf(stderr, "order %lld is too large\n", (long long)n); return 2; }
    std::vector<double> in((size_t)(eig ? n * n : n));
    if (fread(in.data(), sizeof(double), in.size(), f) != in.size()) { fprintf(stderr, "short input\n"); return 2; }
    fclose(f);
    std::vector<double> out;
    if (eig) {
        out.resize((size_t)(n + n * n + 1));
        out[(size_t)(n + n * n)] = (double)mih::sym_eig_jacobi((int)n, in.data(), out.data(), out.data() + n);
    } else if (!strcmp(argv[1], "rank")) {
        out.push_back((double)mih::sym_eig_rank((int)n, in.data()));
    } else if (!strcmp(argv[1], "sign")) {
        out = in;
        mih::sign_rule_apply(n, out.data());
    } else {
        fprintf(stderr, "unknown command %s\n", argv[1]);
        return 2;
    }
    f = fopen(argv[3], "wb");
    if (!f) { perror(argv[3]); return 2; }
    if (fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) { fprintf(stderr, "short output\n"); return 2; }
    fclose(f);
    return 0;
}
