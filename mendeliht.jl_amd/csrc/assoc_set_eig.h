// assoc_set_eig.h -- the device code that the eigenvalue kernels of the set pass share (assoc_sets.hip: k_assoc_set_eig, the
// eigenvalues of M; assoc_skato.hip: k_assoc_set_rho, those of M_rho and M~): the entries of M, the fixed-tree sum of a workgroup
// and the parallel-order Jacobi iteration itself.  One copy, so that the eigenvalues of M_0 = M are those of M bit for bit.
#pragma once
#include "common.h"
#include "sym_eig.h"
#include <limits>

namespace mih {

constexpr int kSetEigLds = 64;                   // a set of up to 64 members has its matrix in LDS; a larger one in a global slab

// M_jk for j >= k is (omega_j K_jk) omega_k, mirrored: one value for both triangles
__device__ __forceinline__ double set_m_entry(const double *K, int m, const double *om, int j, int k)
{
#pragma clang fp contract(off)
    return j >= k ? (om[j] * K[j * m + k]) * om[k] : (om[k] * K[k * m + j]) * om[j];
}

// red[0] becomes the sum of the 256 values over the fixed tree; every thread gets it
__device__ __forceinline__ double set_block_sum(double *red, double v)
{
#pragma clang fp contract(off)
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + k];
        __syncthreads();
    }
    return red[0];
}

// The eigenvalues of the symmetric matrix a (order m; stored with the order me = m rounded up to even, a zero row and column
// padding an odd m, lda doubles between rows; LDS or global), descending, every value <= 0 set to 0, into lam[0 .. m).  Called by
// all 256 threads of a workgroup; f2 is the thread's share of sum a_ij^2 (its idx = tid, tid + 256, .. of the me x me entries, in
// that order).  a is destroyed.
// Two-sided Jacobi with the round-robin parallel ordering: me - 1 steps a sweep, step t pairing (me - 1, t) and
// ((t + k) mod (me - 1), (t - k) mod (me - 1)), k = 1 .. me / 2 - 1.  A step computes the me / 2 rotations from the matrix as it
// stands (sym_eig_jacobi's expressions; a pair at or below u |a|_F / m is left alone), then every 2 x 2 block (pair A, pair B),
// B <= A, is transformed by ONE thread, Z = J_A' (X J_B), and mirrored; the diagonal block becomes
// diag(a_pp - t a_pq, a_qq + t a_pq).  A sweep ends the iteration when the off-diagonal norm has fallen to u |a|_F
// (sym_eig_jacobi's rule), kSymEigMaxSweeps at most; a NaN or an infinity in a gives all NaN.  The order of the rotations and of
// every sum is fixed and contraction is off: the values are reproducible bit for bit.
__device__ __forceinline__ void set_jacobi_eig(double *a, int lda, int m, double f2, double *lam)
{
#pragma clang fp contract(off)
    __shared__ double red[256];
    __shared__ double dg[kSymEigMaxOrder];
    __shared__ double rc[kSymEigMaxOrder / 2], rsn[kSymEigMaxOrder / 2], rd0[kSymEigMaxOrder / 2], rd1[kSymEigMaxOrder / 2];
    __shared__ int rp[kSymEigMaxOrder / 2], rq[kSymEigMaxOrder / 2], rv[kSymEigMaxOrder / 2];
    const int tid = threadIdx.x, me = (m + 1) & ~1, h = me / 2;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const double fro = sqrt(set_block_sum(red, f2));
    if (!(fro <= std::numeric_limits<double>::max())) {              // a NaN or an infinity: nothing to decompose
        if (tid < m) lam[tid] = nan;
        return;
    }
    const double u = 1.1102230246251565e-16, skip = u * fro / (double)m;
    for (int sweeps = 0;; ++sweeps) {
        double o2 = 0.0;
        for (int idx = tid; idx < me * me; idx += 256) {
            const int i = idx / me, j = idx % me;
            if (i != j) o2 = o2 + a[i * lda + j] * a[i * lda + j];
        }
        const double off = sqrt(set_block_sum(red, o2));
        if (off <= u * fro || sweeps == kSymEigMaxSweeps) break;
        for (int t = 0; t < me - 1; ++t) {
            if (tid < h) {
                int p = tid == 0 ? me - 1 : (t + tid) % (me - 1), q = tid == 0 ? t : (t - tid + (me - 1)) % (me - 1);
                if (p > q) { const int x = p; p = q; q = x; }
                const double apq = a[p * lda + q], app = a[p * lda + p], aqq = a[q * lda + q];
                const bool on = fabs(apq) > skip;
                double cc = 1.0, sn = 0.0, tp = 0.0;
                if (on) {
                    const double theta = (aqq - app) / (2.0 * apq);
                    const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + hypot(theta, 1.0));
                    cc = 1.0 / hypot(tt, 1.0); sn = tt * cc; tp = tt * apq;
                }
                rp[tid] = p; rq[tid] = q; rv[tid] = on ? 1 : 0; rc[tid] = cc; rsn[tid] = sn; rd0[tid] = app - tp; rd1[tid] = aqq + tp;
            }
            __syncthreads();
            for (int idx = tid; idx < h * h; idx += 256) {
                const int A = idx / h, B = idx % h;
                if (B > A) continue;
                const int pa = rp[A], qa = rq[A], pb = rp[B], qb = rq[B];
                if (A == B) {
                    if (rv[A]) { a[pa * lda + pa] = rd0[A]; a[qa * lda + qa] = rd1[A]; a[pa * lda + qa] = 0.0; a[qa * lda + pa] = 0.0; }
                    continue;
                }
                if (!rv[A] && !rv[B]) continue;
                const double ca = rc[A], sa_ = rsn[A], cb = rc[B], sb = rsn[B];
                const double xpp = a[pa * lda + pb], xpq = a[pa * lda + qb], xqp = a[qa * lda + pb], xqq = a[qa * lda + qb];
                const double ypp = cb * xpp - sb * xpq, ypq = sb * xpp + cb * xpq, yqp = cb * xqp - sb * xqq, yqq = sb * xqp + cb * xqq;
                const double zpp = ca * ypp - sa_ * yqp, zqp = sa_ * ypp + ca * yqp, zpq = ca * ypq - sa_ * yqq, zqq = sa_ * ypq + ca * yqq;
                a[pa * lda + pb] = zpp; a[pb * lda + pa] = zpp;
                a[pa * lda + qb] = zpq; a[qb * lda + pa] = zpq;
                a[qa * lda + pb] = zqp; a[pb * lda + qa] = zqp;
                a[qa * lda + qb] = zqq; a[qb * lda + qa] = zqq;
            }
            __syncthreads();
        }
    }
    __syncthreads();
    if (tid < m) dg[tid] = a[tid * lda + tid];
    __syncthreads();
    if (tid < m) {                                                     // descending, equal values by index
        const double d = dg[tid];
        int rank = 0;
        for (int j = 0; j < m; ++j) rank += (dg[j] > d || (dg[j] == d && j < tid)) ? 1 : 0;
        lam[rank] = d > 0.0 ? d : (d == d ? 0.0 : d);
    }
}

}  // namespace mih
