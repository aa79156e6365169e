// ipm_device.hip -- HSD and path-following iterations on gfx950.
//
// Fused O(m+n) kernels (HBM-bound; coalesced CSR/CSC gathers, one pass per
// phase) + the KKT factor/solve of kkt_device.hip.  Per iteration the host
// reads back only the scalars the reference prints or branches on.
//
// Sharded (block-angular, ipm.h ShardSpec): the same kernels run on the
// shard's local problem; rows >= mrow (the replicated linking rows) take
// their A x from lax (A_link x summed over the shards), rows >= mcnt are
// left out of the shard's partial sums, and every scalar the host reads is
// allreduced before it is read.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "dev_common.h"
#include "hip_util.h"
#include "ipm.h"
#include "lp_io.h"
#include "value_maps.h"

namespace ipo {

namespace {

constexpr int NT = 256;

__global__ void __launch_bounds__(NT) k_fill(int n, double v, double* __restrict__ a) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i < n) a[i] = v;
}

// ---------------------------------------------------------------- HSD
// rows i < m (hsd.c:182-189, 216, 221, 226):
//   r1 = (A x)_i - b_i phi + w_i ;  ||r1||^2 partial
//   rho = -(1-delta) r1 + w - delta mu / y ;  E = w / y ;  fy = rho ;  gy = -b
// cols j < n (hsd.c:191-198, 215, 220, 225):
//   s1 = -(A'y)_j + c_j phi + z_j ;  ||s1||^2 partial
//   sigma = -(1-delta) s1 + z - delta mu / x ;  D = z / x ;  fx = -sigma ;  gx = -c
__global__ void __launch_bounds__(kResThreads)
k_hsd_residuals(int m, int n, const int* __restrict__ kAt, const int* __restrict__ iAt, const double* __restrict__ At,
                const int* __restrict__ kA, const int* __restrict__ iA, const double* __restrict__ A,
                const double* __restrict__ b, const double* __restrict__ c, const double* __restrict__ x,
                const double* __restrict__ y, const double* __restrict__ w, const double* __restrict__ z, double phi_h,
                double delta, double mu_h, double* __restrict__ E, double* __restrict__ D, double* __restrict__ fy,
                double* __restrict__ fx, double* __restrict__ gy, double* __restrict__ gx, double* __restrict__ part,
                int mrow, int mcnt, const double* __restrict__ lax, const double* __restrict__ phimu) {
    __shared__ double sh[kResThreads / 64];
    // phimu: {phi, mu} computed on the device (scal_'s kIsPhiMu, ipm.h; the
    // overlapped HSD iteration: E and D are then written by k_hsd_scaling
    // ahead of the factorisation)
    const double phi = phimu ? phimu[0] : phi_h;
    const double mu = phimu ? phimu[1] : mu_h;
    const bool wde = phimu == nullptr;
    double sr = 0.0, ss = 0.0;
    for (int i = blockIdx.x * kResThreads + threadIdx.x; i < m + n; i += kRedBlocks * kResThreads) {
        if (i < m) {
            double ax = 0.0;
            if (i >= mrow) ax = lax[i - mrow];      // linking row of a shard: summed over the shards
            else
                ax = sparse_dot(kAt[i], kAt[i + 1], At, iAt, x);
            const double r1 = ax - b[i] * phi + w[i];
            if (i < mcnt) sr += r1 * r1;
            const double rho = -(1 - delta) * r1 + w[i] - delta * mu / y[i];
            if (wde) E[i] = w[i] / y[i];
            fy[i] = rho;
            gy[i] = -b[i];
        } else {
            const int j = i - m;
            double aty = 0.0;
            aty = sparse_dot(kA[j], kA[j + 1], A, iA, y);
            const double s1 = -aty + c[j] * phi + z[j];
            ss += s1 * s1;
            const double sg = -(1 - delta) * s1 + z[j] - delta * mu / x[j];
            if (wde) D[j] = z[j] / x[j];
            fx[j] = -sg;
            gx[j] = -c[j];
        }
    }
    sr = block_sum_w<kResThreads / 64>(sr, sh);
    ss = block_sum_w<kResThreads / 64>(ss, sh);
    if (threadIdx.x == 0) { part[blockIdx.x] = sr; part[kRedBlocks + blockIdx.x] = ss; }
}

// directions + ratio test (hsd.c:233-237, 249-256); dphip: scal_'s kIsDphi
__global__ void __launch_bounds__(NT)
k_hsd_directions(int m, int n, const double* __restrict__ dphip, double delta, double mu, const double* __restrict__ fx,
                 const double* __restrict__ gx, const double* __restrict__ fy, const double* __restrict__ gy,
                 const double* __restrict__ x, const double* __restrict__ z, const double* __restrict__ y,
                 const double* __restrict__ w, const double* __restrict__ D, const double* __restrict__ E,
                 double* __restrict__ dx, double* __restrict__ dz, double* __restrict__ dy, double* __restrict__ dw,
                 double* __restrict__ part) {
    __shared__ double sh[4];
    const double dphi = *dphip;
    double th = 0.0;
    for (int i = blockIdx.x * NT + threadIdx.x; i < m + n; i += kRedBlocks * NT) {
        if (i < n) {
            const double ddx = fx[i] - gx[i] * dphi;
            const double ddz = delta * mu / x[i] - z[i] - D[i] * ddx;
            dx[i] = ddx; dz[i] = ddz;
            th = fmax(th, -ddx / x[i]);
            th = fmax(th, -ddz / z[i]);
        } else {
            const int j = i - n;
            const double ddy = fy[j] - gy[j] * dphi;
            const double ddw = delta * mu / y[j] - w[j] - E[j] * ddy;
            dy[j] = ddy; dw[j] = ddw;
            th = fmax(th, -ddy / y[j]);
            th = fmax(th, -ddw / w[j]);
        }
    }
    th = block_max(th, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = th;
}

__global__ void __launch_bounds__(NT)
k_step(int m, int n, double theta_h, const double* __restrict__ thetap, double* __restrict__ x,
       const double* __restrict__ dx, double* __restrict__ z, const double* __restrict__ dz, double* __restrict__ y,
       const double* __restrict__ dy, double* __restrict__ w, const double* __restrict__ dw) {
    const double theta = thetap ? *thetap : theta_h;     // device-computed step (hsd: kIsTheta) or the host's
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i < n) { x[i] = x[i] + theta * dx[i]; z[i] = z[i] + theta * dz[i]; }
    else if (i < n + m) { const int j = i - n; y[j] = y[j] + theta * dy[j]; w[j] = w[j] + theta * dw[j]; }
}

// E = w / y, D = z / x (hsd.c:188-189; the same divisions as k_hsd_residuals)
__global__ void __launch_bounds__(NT)
k_hsd_scaling(int m, int n, const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ w,
              const double* __restrict__ z, double* __restrict__ E, double* __restrict__ D) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i < m) E[i] = w[i] / y[i];
    else if (i < m + n) { const int j = i - m; D[j] = z[j] / x[j]; }
}

// (sc: IpmSolver::scal_, its slots by name: ipm.h)
// mu of hsd.c:168 on the device, the host's expression: reads kIsZx, kIsWy
// (the dots z'x, w'y) and phi / psi from kIsPhiNext (dev != 0) or the
// arguments; writes kIsPhiMu = phi, mu (the residual kernel's phimu)
__global__ void k_hsd_mu(double* sc, double denom, double phi_h, double psi_h, int dev) {
    const double phi = dev ? sc[kIsPhiNext] : phi_h, psi = dev ? sc[kIsPhiNext + 1] : psi_h;
    sc[kIsPhiMu] = phi;
    sc[kIsPhiMu + 1] = (sc[kIsZx] + sc[kIsWy] + phi * psi) / denom;
}

// hsd.c:226-231 on the device (same operations and order as the host code
// it replaces): reads kIsRed's c'fx, b'fy, c'gx, b'gy; writes kIsDphi = dphi, dpsi
__global__ void k_hsd_dphi(double* sc, double gamma, double delta, double mu, double phi, double psi) {
    const double* red = sc + kIsRed;
    const double dphi = (red[0] - red[1] + gamma) / (red[2] - red[3] - psi / phi);
    const double dpsi = delta * mu / phi - psi - (psi / phi) * dphi;
    sc[kIsDphi] = dphi;
    sc[kIsDphi + 1] = dpsi;
}

// hsd.c:249-266: step length from the largest ratio (kIsRed's first) and
// kIsDphi; writes kIsTheta and kIsPhiNext, the next phi / psi (read by the
// host at the next iteration's synchronisation)
__global__ void k_hsd_theta(double* sc, double phi, double psi) {
    const double dphi = sc[kIsDphi], dpsi = sc[kIsDphi + 1];
    double theta = sc[kIsRed];
    if (theta < -dphi / phi) theta = -dphi / phi;
    if (theta < -dpsi / psi) theta = -dpsi / psi;
    theta = (0.95 / theta > 1.0) ? 1.0 : 0.95 / theta;
    sc[kIsTheta] = theta;
    sc[kIsPhiNext] = phi + theta * dphi;
    sc[kIsPhiNext + 1] = psi + theta * dpsi;
}

__global__ void __launch_bounds__(NT)
k_unscale(int m, int n, double phi, double* __restrict__ x, double* __restrict__ z, double* __restrict__ y,
          double* __restrict__ w) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i < n) { x[i] /= phi; z[i] /= phi; }
    else if (i < n + m) { const int j = i - n; y[j] /= phi; w[j] /= phi; }
}

// ---------------------------------------------------------------- hsdls
// hsdls.c:298-336: largest step keeping x z >= (1-beta) mu along the direction
__device__ __forceinline__ double ls_step(double xj, double zj, double dxj, double dzj, double beta, double delta,
                                          double mu) {
    const double a = dxj * dzj;
    const double b = zj * dxj + xj * dzj + (1 - beta) * (1 - delta) * mu;
    const double c = xj * zj - (1 - beta) * mu;
    const double d = b * b - 4 * a * c;
    if (a == 0.0) return -c / b;
    if (a > 0) {
        if (b < 0) {
            if (d >= 0) return 2 * c / (-b + sqrt(d));
            return HUGE_VAL;
        }
        return HUGE_VAL;
    }
    if (b < 0) return 2 * c / (-b + sqrt(d));
    return (-b - sqrt(d)) / (2 * a);
}

// directions (hsdls.c:209-215) + the linesearch minimum (hsdls.c:221-230),
// returned as a max of -step so the common max finisher applies
__global__ void __launch_bounds__(NT)
k_hsdls_directions(int m, int n, double dphi, double beta, double delta, double mu, const double* __restrict__ fx,
                   const double* __restrict__ gx, const double* __restrict__ fy, const double* __restrict__ gy,
                   const double* __restrict__ x, const double* __restrict__ z, const double* __restrict__ y,
                   const double* __restrict__ w, const double* __restrict__ D, const double* __restrict__ E,
                   double* __restrict__ dx, double* __restrict__ dz, double* __restrict__ dy, double* __restrict__ dw,
                   double* __restrict__ part) {
    __shared__ double sh[4];
    double th = -HUGE_VAL;
    for (int i = blockIdx.x * NT + threadIdx.x; i < m + n; i += kRedBlocks * NT) {
        if (i < n) {
            const double ddx = fx[i] - gx[i] * dphi;
            const double ddz = delta * mu / x[i] - z[i] - D[i] * ddx;
            dx[i] = ddx; dz[i] = ddz;
            th = fmax(th, -ls_step(x[i], z[i], ddx, ddz, beta, delta, mu));
        } else {
            const int j = i - n;
            const double ddy = fy[j] - gy[j] * dphi;
            const double ddw = delta * mu / y[j] - w[j] - E[j] * ddy;
            dy[j] = ddy; dw[j] = ddw;
            th = fmax(th, -ls_step(y[j], w[j], ddy, ddw, beta, delta, mu));
        }
    }
    th = block_max(th, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = th;
}

// ---------------------------------------------------------------- intpt
// rho = b - A x - w, sigma = c - A'y + z and their squared norms (intpt.c:139-149)
__global__ void __launch_bounds__(kResThreads)
k_pf_residuals(int m, int n, const int* __restrict__ kAt, const int* __restrict__ iAt, const double* __restrict__ At,
               const int* __restrict__ kA, const int* __restrict__ iA, const double* __restrict__ A,
               const double* __restrict__ b, const double* __restrict__ c, const double* __restrict__ x,
               const double* __restrict__ y, const double* __restrict__ w, const double* __restrict__ z,
               double* __restrict__ rho, double* __restrict__ sig, double* __restrict__ part, int mrow, int mcnt,
               const double* __restrict__ lax) {
    __shared__ double sh[kResThreads / 64];
    double sr = 0.0, ss = 0.0;
    for (int i = blockIdx.x * kResThreads + threadIdx.x; i < m + n; i += kRedBlocks * kResThreads) {
        if (i < m) {
            double ax = 0.0;
            if (i >= mrow) ax = lax[i - mrow];      // linking row of a shard: summed over the shards
            else
                ax = sparse_dot(kAt[i], kAt[i + 1], At, iAt, x);
            const double r = b[i] - ax - w[i];
            rho[i] = r;
            if (i < mcnt) sr += r * r;
        } else {
            const int j = i - m;
            double aty = 0.0;
            aty = sparse_dot(kA[j], kA[j + 1], A, iA, y);
            const double s = c[j] - aty + z[j];
            sig[j] = s;
            ss += s * s;
        }
    }
    sr = block_sum_w<kResThreads / 64>(sr, sh);
    ss = block_sum_w<kResThreads / 64>(ss, sh);
    if (threadIdx.x == 0) { part[blockIdx.x] = sr; part[kRedBlocks + blockIdx.x] = ss; }
}

// D, E and the right-hand side (intpt.c:194-200)
__global__ void __launch_bounds__(NT)
k_pf_rhs(int m, int n, double mu, const double* __restrict__ x, const double* __restrict__ z,
         const double* __restrict__ y, const double* __restrict__ w, const double* __restrict__ rho,
         const double* __restrict__ sig, double* __restrict__ D, double* __restrict__ E, double* __restrict__ dx,
         double* __restrict__ dy) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i < n) { D[i] = z[i] / x[i]; dx[i] = sig[i] - z[i] + mu / x[i]; }
    else if (i < n + m) { const int j = i - n; E[j] = w[j] / y[j]; dy[j] = rho[j] + w[j] - mu / y[j]; }
}

// dz, dw and the ratio test (intpt.c:204-219)
__global__ void __launch_bounds__(NT)
k_pf_directions(int m, int n, double mu, const double* __restrict__ x, const double* __restrict__ z,
                const double* __restrict__ y, const double* __restrict__ w, const double* __restrict__ D,
                const double* __restrict__ E, const double* __restrict__ dx, const double* __restrict__ dy,
                double* __restrict__ dz, double* __restrict__ dw, double* __restrict__ part) {
    __shared__ double sh[4];
    double th = 0.0;
    for (int i = blockIdx.x * NT + threadIdx.x; i < m + n; i += kRedBlocks * NT) {
        if (i < n) {
            const double v = mu / x[i] - z[i] - D[i] * dx[i];
            dz[i] = v;
            th = fmax(th, -dx[i] / x[i]);
            th = fmax(th, -v / z[i]);
        } else {
            const int j = i - n;
            const double v = mu / y[j] - w[j] - E[j] * dy[j];
            dw[j] = v;
            th = fmax(th, -dy[j] / y[j]);
            th = fmax(th, -v / w[j]);
        }
    }
    th = block_max(th, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = th;
}

// ---------------------------------------------------------------- qp
// k_pf_residuals with the quadratic term: for column j, (Q x)_j over Q's
// column j (= its row j: Q is symmetric) in row order, kept in qx for the
// objectives' x'Qx and subtracted last, sigma = ((c - A'y) + z) - Q x.  One
// thread walks a column of Q serially (sparse_dot), but a column of at least
// qthr > 0 entries (KktDevice::q_long_min) is read from qx, where
// KktDevice::launch_q_long has summed it by one wave beforehand (dense and
// arrow Q).  Not sharded: no mcnt.
__global__ void __launch_bounds__(kResThreads)
k_qp_residuals(int m, int n, const int* __restrict__ kAt, const int* __restrict__ iAt, const double* __restrict__ At,
               const int* __restrict__ kA, const int* __restrict__ iA, const double* __restrict__ A,
               const int* __restrict__ kQ, const int* __restrict__ iQ, const double* __restrict__ Q,
               const double* __restrict__ b, const double* __restrict__ c, const double* __restrict__ x,
               const double* __restrict__ y, const double* __restrict__ w, const double* __restrict__ z,
               double* __restrict__ rho, double* __restrict__ sig, double* __restrict__ qx, double* __restrict__ part,
               int mrow, const double* __restrict__ lax, int qthr) {
    __shared__ double sh[kResThreads / 64];
    double sr = 0.0, ss = 0.0;
    for (int i = blockIdx.x * kResThreads + threadIdx.x; i < m + n; i += kRedBlocks * kResThreads) {
        if (i < m) {
            double ax = 0.0;
            if (i >= mrow) ax = lax[i - mrow];      // A x formed column-blocked beforehand (row_ax)
            else
                ax = sparse_dot(kAt[i], kAt[i + 1], At, iAt, x);
            const double r = b[i] - ax - w[i];
            rho[i] = r;
            sr += r * r;
        } else {
            const int j = i - m;
            const double aty = sparse_dot(kA[j], kA[j + 1], A, iA, y);
            const double q = q_col_long(kQ, j, qthr) ? qx[j] : sparse_dot(kQ[j], kQ[j + 1], Q, iQ, x);
            const double s = ((c[j] - aty) + z[j]) - q;
            qx[j] = q;
            sig[j] = s;
            ss += s * s;
        }
    }
    sr = block_sum_w<kResThreads / 64>(sr, sh);
    ss = block_sum_w<kResThreads / 64>(ss, sh);
    if (threadIdx.x == 0) { part[blockIdx.x] = sr; part[kRedBlocks + blockIdx.x] = ss; }
}

// k_pf_rhs for the factor with the roles of x and y swapped (run_qp): the
// same D, E and right-hand sides, the x block's negated -- the solve then
// leaves dx in dx and -dy in dy
__global__ void __launch_bounds__(NT)
k_qp_rhs(int m, int n, double mu, const double* __restrict__ x, const double* __restrict__ z,
         const double* __restrict__ y, const double* __restrict__ w, const double* __restrict__ rho,
         const double* __restrict__ sig, double* __restrict__ D, double* __restrict__ E, double* __restrict__ dx,
         double* __restrict__ dy) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i < n) { D[i] = z[i] / x[i]; dx[i] = -(sig[i] - z[i] + mu / x[i]); }
    else if (i < n + m) { const int j = i - n; E[j] = w[j] / y[j]; dy[j] = rho[j] + w[j] - mu / y[j]; }
}

// k_pf_directions reading the swapped solve's dy (negated, and stored back
// with its sign for k_step); dz = mu / x - z - D dx with D alone, not D + Q
__global__ void __launch_bounds__(NT)
k_qp_directions(int m, int n, double mu, const double* __restrict__ x, const double* __restrict__ z,
                const double* __restrict__ y, const double* __restrict__ w, const double* __restrict__ D,
                const double* __restrict__ E, const double* __restrict__ dx, double* __restrict__ dy,
                double* __restrict__ dz, double* __restrict__ dw, double* __restrict__ part) {
    __shared__ double sh[4];
    double th = 0.0;
    for (int i = blockIdx.x * NT + threadIdx.x; i < m + n; i += kRedBlocks * NT) {
        if (i < n) {
            const double v = mu / x[i] - z[i] - D[i] * dx[i];
            dz[i] = v;
            th = fmax(th, -dx[i] / x[i]);
            th = fmax(th, -v / z[i]);
        } else {
            const int j = i - n;
            const double ddy = -dy[j];
            const double v = mu / y[j] - w[j] - E[j] * ddy;
            dy[j] = ddy;
            dw[j] = v;
            th = fmax(th, -ddy / y[j]);
            th = fmax(th, -v / w[j]);
        }
    }
    th = block_max(th, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = th;
}

// ---------------------------------------------------------------- pc
// Mehrotra's predictor-corrector (run_pc).  SW: the solver holds the factor
// with the roles of x and y swapped (a solver with Q, as run_qp): the x
// block's right-hand side goes in negated and the solve leaves -dy.
//
// Right-hand sides of the Newton system: rho + w - cy / y for the rows,
// sigma - z + cx / x for the columns, with the centring terms
// cx = mu - dxa dza, cy = mu - dya dwa when mup (scal_'s kIsPcMu) is given;
// without it the predictor's, which also writes D = z / x and E = w / y.
template <bool SW>
__global__ void __launch_bounds__(NT)
k_pc_rhs(int m, int n, const double* __restrict__ mup, const double* __restrict__ x, const double* __restrict__ z,
         const double* __restrict__ y, const double* __restrict__ w, const double* __restrict__ rho,
         const double* __restrict__ sig, double* __restrict__ D, double* __restrict__ E,
         const double* __restrict__ dxa, const double* __restrict__ dza, const double* __restrict__ dya,
         const double* __restrict__ dwa, double* __restrict__ fx, double* __restrict__ fy) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i < n) {
        double v = sig[i] - z[i];
        if (mup) v += (*mup - dxa[i] * dza[i]) / x[i];
        else D[i] = z[i] / x[i];
        fx[i] = SW ? -v : v;
    } else if (i < n + m) {
        const int j = i - n;
        double v = rho[j] + w[j];
        if (mup) v -= (*mup - dya[j] * dwa[j]) / y[j];
        else E[j] = w[j] / y[j];
        fy[j] = v;
    }
}

// the predictor's dza = -z - D dxa, dwa = -w - E dya and its ratio test (dya
// stored back with its sign when SW)
template <bool SW>
__global__ void __launch_bounds__(NT)
k_pc_affine(int m, int n, const double* __restrict__ x, const double* __restrict__ z, const double* __restrict__ y,
            const double* __restrict__ w, const double* __restrict__ D, const double* __restrict__ E,
            const double* __restrict__ dxa, double* __restrict__ dya, double* __restrict__ dza,
            double* __restrict__ dwa, double* __restrict__ part) {
    __shared__ double sh[4];
    double th = 0.0;
    for (int i = blockIdx.x * NT + threadIdx.x; i < m + n; i += kRedBlocks * NT) {
        if (i < n) {
            const double v = -z[i] - D[i] * dxa[i];
            dza[i] = v;
            th = fmax(th, -dxa[i] / x[i]);
            th = fmax(th, -v / z[i]);
        } else {
            const int j = i - n;
            const double ddy = SW ? -dya[j] : dya[j];
            const double v = -w[j] - E[j] * ddy;
            if (SW) dya[j] = ddy;
            dwa[j] = v;
            th = fmax(th, -ddy / y[j]);
            th = fmax(th, -v / w[j]);
        }
    }
    th = block_max(th, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = th;
}

// the corrected dz = cx / x - z - D dx, dw = cy / y - w - E dy and their
// ratio test (dy stored back with its sign when SW); mup: kIsPcMu
template <bool SW>
__global__ void __launch_bounds__(NT)
k_pc_directions(int m, int n, const double* __restrict__ mup, const double* __restrict__ x,
                const double* __restrict__ z, const double* __restrict__ y, const double* __restrict__ w,
                const double* __restrict__ D, const double* __restrict__ E, const double* __restrict__ dxa,
                const double* __restrict__ dza, const double* __restrict__ dya, const double* __restrict__ dwa,
                const double* __restrict__ dx, double* __restrict__ dy, double* __restrict__ dz,
                double* __restrict__ dw, double* __restrict__ part) {
    __shared__ double sh[4];
    const double mu = *mup;
    double th = 0.0;
    for (int i = blockIdx.x * NT + threadIdx.x; i < m + n; i += kRedBlocks * NT) {
        if (i < n) {
            const double v = (mu - dxa[i] * dza[i]) / x[i] - z[i] - D[i] * dx[i];
            dz[i] = v;
            th = fmax(th, -dx[i] / x[i]);
            th = fmax(th, -v / z[i]);
        } else {
            const int j = i - n;
            const double ddy = SW ? -dy[j] : dy[j];
            const double v = (mu - dya[j] * dwa[j]) / y[j] - w[j] - E[j] * ddy;
            if (SW) dy[j] = ddy;
            dw[j] = v;
            th = fmax(th, -ddy / y[j]);
            th = fmax(th, -v / w[j]);
        }
    }
    th = block_max(th, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = th;
}

// The centring parameter on the device: reads the predictor's largest ratio
// (kIsPcRatio), the six dots of kIsPcDots and gamma's two (kIsZx, kIsWy, the
// host's sum); theta_a = 1 if t <= 1 else 1 / t, gamma_a = gamma + theta_a
// (g1 + theta_a g2), s = min(1, max(0, gamma_a / gamma))^3; writes kIsPcMu =
// s gamma / denom
__global__ void k_pc_mu(double* sc, double denom) {
    const double t = sc[kIsPcRatio];
    const double ta = t <= 1.0 ? 1.0 : 1.0 / t;
    const double* d = sc + kIsPcDots;
    const double gamma = sc[kIsZx] + sc[kIsWy];
    const double g1 = d[0] + d[1] + d[2] + d[3], g2 = d[4] + d[5];
    const double ga = gamma + ta * (g1 + ta * g2);
    const double s = fmin(1.0, fmax(0.0, ga / gamma));
    sc[kIsPcMu] = s * s * s * gamma / denom;
}

// theta = min(1, 0.95 / t) from the corrected directions' largest ratio
// (kIsRed's first), 1 if t = 0; writes kIsTheta
__global__ void k_pc_theta(double* sc) {
    const double t = sc[kIsRed];
    sc[kIsTheta] = (t == 0.0 || 0.95 / t > 1.0) ? 1.0 : 0.95 / t;
}

// ---------------------------------------------------------------- the Mehrotra start
// IpmSolver::mehrotra_start, SW as above.  The factor's
// D = E = 1 and the two systems' right-hand sides, (fy, fx) = (b, 0) into
// (by, bx) and (0, c) into (cy, cx), the x block's negated when SW.
template <bool SW>
__global__ void __launch_bounds__(NT)
k_ms_fill(int m, int n, const double* __restrict__ b, const double* __restrict__ c, double* __restrict__ D,
          double* __restrict__ E, double* __restrict__ bx, double* __restrict__ by, double* __restrict__ cx,
          double* __restrict__ cy) {
    for (int i = blockIdx.x * NT + threadIdx.x; i < m + n; i += kRedBlocks * NT) {
        if (i < n) {
            D[i] = 1.0;
            bx[i] = 0.0;
            cx[i] = SW ? -c[i] : c[i];
        } else {
            const int j = i - n;
            E[j] = 1.0;
            by[j] = b[j];
            cy[j] = 0.0;
        }
    }
}

// The two solutions unpacked: x~ = dx, w~ = -dy of the first system, y~ = dy,
// z~ = -dx of the second (the swapped solve leaves -dy where the LP's leaves
// dy).  part: kRedBlocks partials each of max(-x~, -w~) and max(-y~, -z~),
// the two minima negated so the common max finisher applies.
template <bool SW>
__global__ void __launch_bounds__(NT)
k_ms_unpack(int m, int n, const double* __restrict__ bx, const double* __restrict__ by, const double* __restrict__ cx,
            const double* __restrict__ cy, double* __restrict__ x, double* __restrict__ w, double* __restrict__ y,
            double* __restrict__ z, double* __restrict__ part) {
    __shared__ double sh[4];
    double np = -HUGE_VAL, nd = -HUGE_VAL;
    for (int i = blockIdx.x * NT + threadIdx.x; i < m + n; i += kRedBlocks * NT) {
        if (i < n) {
            const double xv = bx[i], zv = -cx[i];
            x[i] = xv; z[i] = zv;
            np = fmax(np, -xv);
            nd = fmax(nd, -zv);
        } else {
            const int j = i - n;
            const double wv = SW ? by[j] : -by[j], yv = SW ? -cy[j] : cy[j];
            w[j] = wv; y[j] = yv;
            np = fmax(np, -wv);
            nd = fmax(nd, -yv);
        }
    }
    np = block_max(np, sh);
    nd = block_max(nd, sh);
    if (threadIdx.x == 0) { part[blockIdx.x] = np; part[kRedBlocks + blockIdx.x] = nd; }
}

// delta_p = max(0, -1.5 min(x~, w~)), delta_d = max(0, -1.5 min(y~, z~));
// reads kIsMsNegMin, writes kIsMsDelta
__global__ void k_ms_delta(double* sc) {
    sc[kIsMsDelta] = fmax(0.0, 1.5 * sc[kIsMsNegMin]);
    sc[kIsMsDelta + 1] = fmax(0.0, 1.5 * sc[kIsMsNegMin + 1]);
}

// x, w += sh[0], y, z += sh[1].  With part: the shift by kIsMsDelta, and
// kRedBlocks partials each of g = x'z + w'y, Sp = sum x + sum w and Sd =
// sum z + sum y of the shifted point: a thread's entries in index order, the
// block's by block_sum's tree, so the sums have the same bits on every run.
// Without: the shift by kIsMsEps.
__global__ void __launch_bounds__(NT)
k_ms_shift(int m, int n, const double* __restrict__ sh2, double* __restrict__ x, double* __restrict__ w,
           double* __restrict__ y, double* __restrict__ z, double* __restrict__ part) {
    __shared__ double sh[4];
    const double sp = sh2[0], sd = sh2[1];
    double g = 0.0, Sp = 0.0, Sd = 0.0;
    for (int i = blockIdx.x * NT + threadIdx.x; i < m + n; i += kRedBlocks * NT) {
        if (i < n) {
            const double xv = x[i] + sp, zv = z[i] + sd;
            x[i] = xv; z[i] = zv;
            g += xv * zv; Sp += xv; Sd += zv;
        } else {
            const int j = i - n;
            const double wv = w[j] + sp, yv = y[j] + sd;
            w[j] = wv; y[j] = yv;
            g += wv * yv; Sp += wv; Sd += yv;
        }
    }
    if (!part) return;
    g = block_sum(g, sh);
    Sp = block_sum(Sp, sh);
    Sd = block_sum(Sd, sh);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = g;
        part[kRedBlocks + blockIdx.x] = Sp;
        part[2 * kRedBlocks + blockIdx.x] = Sd;
    }
}

// eps_p = g / (2 Sd), eps_d = g / (2 Sp) if g, Sp and Sd are all > 0, else
// both 1 (b = 0 and c = 0); reads kIsMsSums, writes kIsMsEps
__global__ void k_ms_eps(double* sc) {
    const double g = sc[kIsMsSums], Sp = sc[kIsMsSums + 1], Sd = sc[kIsMsSums + 2];
    const bool ok = g > 0.0 && Sp > 0.0 && Sd > 0.0;
    sc[kIsMsEps] = ok ? g / (2.0 * Sd) : 1.0;
    sc[kIsMsEps + 1] = ok ? g / (2.0 * Sp) : 1.0;
}

// host copy of ls_step for the (phi, psi) pair (hsdls.c:229)
double ls_step_host(double xj, double zj, double dxj, double dzj, double beta, double delta, double mu) {
    const double a = dxj * dzj;
    const double b = zj * dxj + xj * dzj + (1 - beta) * (1 - delta) * mu;
    const double c = xj * zj - (1 - beta) * mu;
    const double d = b * b - 4 * a * c;
    if (a == 0.0) return -c / b;
    if (a > 0) return (b < 0 && d >= 0) ? 2 * c / (-b + std::sqrt(d)) : HUGE_VAL;
    if (b < 0) return 2 * c / (-b + std::sqrt(d));
    return (-b - std::sqrt(d)) / (2 * a);
}

double now_s() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

const char* kHsdHeader =
    "--------------------------------------------------------------------------\n"
    "         |           Primal          |            Dual           |       |\n"
    "  Iter   |  Obj Value       Infeas   |  Obj Value       Infeas   |  mu   |\n"
    "- - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - \n";
const char* kIntptHeader =
    "------------------------------------------------------------------\n"
    "         |           Primal          |            Dual           |\n"
    "  Iter   |  Obj Value       Infeas   |  Obj Value       Infeas   |\n"
    "- - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - \n";

}  // namespace

IpmSolver::IpmSolver(int m, int n, const int* kA, const int* iA, const double* A, const double* b, const double* c,
                     double f, hipStream_t stream, const ShardSpec* shard, const QBlock* q)
    : m_(m), n_(n), f_(f), stream_(stream) {
    const double t0 = now_s();
    sharded_ = shard != nullptr;
    has_q_ = q && q->kQ && q->kQ[n] > 0;      // an empty Q is the LP: the LP's own factor
    if (has_q_ && sharded_) throw std::invalid_argument("qp: a solver with Q cannot be sharded");
    mg_ = m;
    ng_ = n;
    nzg_ = kA[n];
    nz_ = kA[n];
    mcnt_ = m;
    if (shard) {
        if (shard->nforced < 0 || shard->nforced > m) throw std::invalid_argument("shard: nforced out of range");
        nforced_ = shard->nforced;
        xch_ = shard->xch;
        if (xch_) {
            mg_ = shard->m_global;
            ng_ = shard->n_global;
            nzg_ = shard->nz_global;
            if (xch_->rank() != 0) mcnt_ = m - nforced_;   // linking rows are counted on rank 0
        }
    }
    // LPs with a vector of kOrderedMaxLen entries (none in netlib) take every
    // dot of theirs in the segmented order; IPO_HIP_DOT_SEGMIN overrides
    dot_segmin_ = knobs_.dot_segmin >= 0 ? knobs_.dot_segmin : std::max(mg_, ng_) >= kOrderedMaxLen ? kSegDotLen : 0;
    if (!stream_) {
        IPO_HIP_CHECK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
        own_stream_ = true;
    }
    if (has_q_) {
        std::vector<int> kat, iat;
        std::vector<double> at;
        csc_transpose(m, n, kA, iA, A, kat, iat, at);
        // KktDevice on A' (n x m): its first block, the one that takes a Q
        // (kkt_device.h QBlock), is then the x block (run_qp)
        QBlock qb = *q;
        qb.qmax = 1;
        kkt_ = std::make_unique<KktDevice>(n, m, kat.data(), iat.data(), at.data(), stream_, 0, &qb);
        // update()'s maps: at = A[ucsr], and Q's transposed entries
        qnz_ = q->kQ[n];
        const std::vector<int> ucsr = csr_value_map(m, n, kA, iA), qt = q_transpose_map(n, q->kQ, q->iQ);
        ucsr_.upload(ucsr, stream_);
        qtmap_.upload(qt, stream_);
        IPO_HIP_CHECK(hipStreamSynchronize(stream_));   // locals
    } else {
        kkt_ = std::make_unique<KktDevice>(m, n, kA, iA, A, stream_, nforced_);
        kkt_->set_exchange(xch_);
    }
    if (dot_segmin_ > 0 && !xch_ && !has_q_) {
        // trailing rows of at least kLongRow entries (the linking rows of a
        // block-angular LP): their serial row products held up the whole
        // refinement residual (1.5 ms a launch on configs[4])
        constexpr int kLongRow = 256;
        std::vector<int> cnt(m > 0 ? m : 1, 0);
        for (int k = 0; k < kA[n]; k++) cnt[iA[k]]++;
        int r0 = m;
        while (r0 > 0 && cnt[r0 - 1] >= kLongRow) r0--;
        if (r0 < m) kkt_->set_long_rows(r0);
    }
    const size_t mm = m > 0 ? m : 1, nn = n > 0 ? n : 1;
    b_.upload(b, m, stream_);
    c_.upload(c, n, stream_);
    for (DevBuf<double>* v : {&x_, &z_, &sig_, &D_, &fx_, &gx_, &dx_, &dz_, &qx_}) v->alloc(nn);
    for (DevBuf<double>* v : {&y_, &w_, &rho_, &E_, &fy_, &gy_, &dy_, &dw_}) v->alloc(mm);
    if (m == 0) b_.alloc(1);
    if (n == 0) c_.alloc(1);
    part_.alloc(8 * kRedBlocks);
    part2_.alloc(8 * kRedBlocks);
    scal_.alloc(kIsCount);
    IPO_HIP_CHECK(hipStreamCreateWithFlags(&side_, hipStreamNonBlocking));
    IPO_HIP_CHECK(hipEventCreateWithFlags(&ev_step_, hipEventDisableTiming));
    IPO_HIP_CHECK(hipEventCreateWithFlags(&ev_side_, hipEventDisableTiming));
    lax_.alloc(nforced_ > 0 ? nforced_ : 1);
    axsliced_ = rows_ax_sliced(knobs_, n_) && !xch_;
    if (axsliced_) {
        ax_.alloc(m_ > 0 ? m_ : 1);
        axplan_.build(m, n, kA, iA, A, knobs_.ax_blocks, stream_);
    }
    IPO_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&hs_), kIsCount * sizeof(double), hipHostMallocDefault));
    IPO_HIP_CHECK(hipStreamSynchronize(stream_));
    t_setup_ = now_s() - t0;
}

IpmSolver::~IpmSolver() {
    if (side_) (void)hipStreamSynchronize(side_);
    if (hs_) (void)hipHostFree(hs_);
    if (ev_step_) (void)hipEventDestroy(ev_step_);
    if (ev_side_) (void)hipEventDestroy(ev_side_);
    if (side_) (void)hipStreamDestroy(side_);
    kkt_.reset();
    if (own_stream_) (void)hipStreamDestroy(stream_);
}

void IpmSolver::reduce(const RedJobs& j, int nout) {
    launch_reduce(j, part_.get(), scal_.get(), stream_);
    xsum(scal_.get(), nout, RedOp::Sum);
    IPO_HIP_CHECK(hipMemcpyAsync(hs_, scal_.get(), nout * sizeof(double), hipMemcpyDeviceToHost, stream_));
    IPO_HIP_CHECK(hipStreamSynchronize(stream_));
}

void IpmSolver::row_ax(const double* x, hipStream_t st) {
    if (!axsliced_) return;
    axplan_.launch(x, ax_.get(), st);
}

void IpmSolver::link_ax(const double* x) {
    row_ax(x, stream_);
    if (!xch_ || nforced_ == 0) return;
    launch_link_ax(m_ - nforced_, m_, kkt_->kAt(), kkt_->iAt(), kkt_->At(), x, lax_.get(), stream_);
    xsum(lax_.get(), nforced_, RedOp::Sum);
}

void IpmSolver::print_dims(FILE* tr) const { std::fprintf(tr, "m = %d,n = %d,nz = %ld\n", mg_, ng_, nzg_); }

void IpmSolver::download(double* x, double* y, double* w, double* z) const {
    if (x) x_.download(x, n_, stream_);
    if (y) y_.download(y, m_, stream_);
    if (w) w_.download(w, m_, stream_);
    if (z) z_.download(z, n_, stream_);
    IPO_HIP_CHECK(hipStreamSynchronize(stream_));
}

int IpmSolver::run(const IpmOptions& opt, IpmResult* res) {
    IpmResult local;
    if (!res) res = &local;
    *res = IpmResult();
    const bool qp = opt.method == Method::Qp;
    if (qp && sharded_) throw std::invalid_argument("qp: not supported on a sharded solver");
    const bool pc = opt.method == Method::Pc;
    if (pc && sharded_) throw std::invalid_argument("pc: not supported on a sharded solver");
    if (!qp && !pc && has_q_) throw std::invalid_argument("a solver built with Q runs method qp only (hsd, intpt and hsdls are LP methods)");
    if (has_start_ && !qp && !pc && opt.method != Method::Intpt)
        throw std::invalid_argument("a start point is set: hsd and hsdls take none (their state includes phi and psi); "
                                    "clear it, or run intpt, qp or pc");
    if (rule_ == StartRule::Mehrotra && !qp && !pc && opt.method != Method::Intpt)
        throw std::invalid_argument("the start rule mehrotra is set: hsd and hsdls take no start point (their state "
                                    "includes phi and psi); set the default rule, or run intpt, qp or pc");
    KktDevice& K = *kkt_;
    res->t_setup_s = t_setup_;
    K.enable_timing(opt.timing);
    K.reset_timers();         // the counters and phase times of this solve only
    K.set_epsdiag(1.0e-14);   // ldlt.c:31: every solve starts from the reference's eps_diag
    const double t0 = now_s();
    // an empty Q is the LP: intpt's iteration on the LP's factor
    const int st = qp                            ? (has_q_ ? run_qp(opt, res) : run_intpt(opt, res))
                   : pc                          ? (has_q_ ? run_pc<true>(opt, res) : run_pc<false>(opt, res))
                   : opt.method == Method::Intpt ? run_intpt(opt, res)
                   : opt.method == Method::Hsdls ? run_hsdls(opt, res)
                                                 : run_hsd(opt, res);
    res->t_solve_s = now_s() - t0;
    res->status = st;
    res->kkt = K.timers();
    ran_ = true;
    return st;
}

void IpmSolver::init_point(double v, IpmResult* res) {
    hipStream_t s = stream_;
    const int m = m_, n = n_;
    if (has_start_) {
        const std::pair<DevBuf<double>*, const DevBuf<double>*> cp[] = {{&x_, &sx_}, {&z_, &sz_}, {&y_, &sy_}, {&w_, &sw_}};
        for (const auto& c : cp) {
            const size_t len = (c.first == &x_ || c.first == &z_) ? n : m;
            if (len) IPO_HIP_CHECK(hipMemcpyAsync(c.first->get(), c.second->get(), len * sizeof(double), hipMemcpyDeviceToDevice, s));
        }
        return;
    }
    if (rule_ == StartRule::Mehrotra) {
        res->refine_passes += mehrotra_start(x_.get(), y_.get(), w_.get(), z_.get());
        // the iteration finds the factor as after a held start: run()'s
        // eps_diag, whatever the start's factorisation grew it to (that
        // factorisation asked for no pre-pass, so none is pending)
        kkt_->set_epsdiag(1.0e-14);
        return;
    }
    for (DevBuf<double>* p : {&x_, &z_}) hipLaunchKernelGGL(k_fill, dim3(ceil_div(n, NT)), dim3(NT), 0, s, n, v, p->get());
    for (DevBuf<double>* p : {&y_, &w_}) hipLaunchKernelGGL(k_fill, dim3(ceil_div(m, NT)), dim3(NT), 0, s, m, v, p->get());
}

namespace {
// the slots of IpmSolver::vfirst_
constexpr int kVfA = 0, kVfB = 1, kVfC = 2, kVfQ = 3, kVfQsym = 4, kVfX = 5, kVfY = 6, kVfW = 7, kVfZ = 8, kVfCount = 9;
constexpr int kVfNone = 0x7f7f7f7f;      // a slot no kernel lowered (memset 0x7f)
}  // namespace

// Mehrotra's start point.  "Solve" is the factor's refined
// solve [-E A; A' D (+ Q)] (dy, dx) = (fy, fx), the LP's own factor or, for
// a solver with Q, the swapped one in run_qp's calling convention.
//   1. E = 1, D = 1, one factorisation
//   2. (fy, fx) = (b, 0): x~ = dx, w~ = -dy, so A x~ + w~ = b at least norm
//      (with Q the norm weighted by I + Q)
//   3. (fy, fx) = (0, c) with the same factor: y~ = dy, z~ = -dx, for an LP
//      A'y~ - z~ = c at least norm
//   4. delta_p = max(0, -1.5 min(x~, w~)) onto x~, w~; delta_d = max(0, -1.5
//      min(y~, z~)) onto y~, z~
//   5. g = x'z + w'y, Sp = sum x + sum w, Sd = sum z + sum y; eps_p =
//      g / (2 Sd) onto x, w and eps_d = g / (2 Sp) onto y, z; both 1 unless
//      g, Sp and Sd are all > 0
// The scalars stay on the device (the kIsMs slots); the one read-back is the
// check that every entry came out finite and > 0.
long IpmSolver::mehrotra_start(double* x, double* y, double* w, double* z) {
    hipStream_t s = stream_;
    const int m = m_, n = n_;
    KktDevice& K = *kkt_;
    double* sc = scal_.get();
    long passes = 0;
    const auto go = [&](auto fill, auto unpack) {
        hipLaunchKernelGGL(fill, dim3(kRedBlocks), dim3(NT), 0, s, m, n, b_.get(), c_.get(), D_.get(), E_.get(), gx_.get(),
                           gy_.get(), dx_.get(), dy_.get());
        if (has_q_) {
            K.factor(D_.get(), E_.get());
            K.solve(D_.get(), E_.get(), gx_.get(), gy_.get());
            passes += K.last_passes();
            K.solve(D_.get(), E_.get(), dx_.get(), dy_.get());
        } else {
            K.factor(E_.get(), D_.get());
            K.solve(E_.get(), D_.get(), gy_.get(), gx_.get());
            passes += K.last_passes();
            K.solve(E_.get(), D_.get(), dy_.get(), dx_.get());
        }
        passes += K.last_passes();
        hipLaunchKernelGGL(unpack, dim3(kRedBlocks), dim3(NT), 0, s, m, n, gx_.get(), gy_.get(), dx_.get(), dy_.get(), x, w,
                           y, z, part_.get());
    };
    if (has_q_) go(k_ms_fill<true>, k_ms_unpack<true>);
    else go(k_ms_fill<false>, k_ms_unpack<false>);
    hipLaunchKernelGGL(k_finish_reduce, dim3(1), dim3(kRedThreads), 0, s, part_.get(), 2, 3u, sc + kIsMsNegMin);
    hipLaunchKernelGGL(k_ms_delta, dim3(1), dim3(1), 0, s, sc);
    hipLaunchKernelGGL(k_ms_shift, dim3(kRedBlocks), dim3(NT), 0, s, m, n, static_cast<const double*>(sc + kIsMsDelta), x,
                       w, y, z, part_.get());
    hipLaunchKernelGGL(k_finish_reduce, dim3(1), dim3(kRedThreads), 0, s, part_.get(), 3, 0u, sc + kIsMsSums);
    hipLaunchKernelGGL(k_ms_eps, dim3(1), dim3(1), 0, s, sc);
    hipLaunchKernelGGL(k_ms_shift, dim3(kRedBlocks), dim3(NT), 0, s, m, n, static_cast<const double*>(sc + kIsMsEps), x, w,
                       y, z, static_cast<double*>(nullptr));
    if (vfirst_.size() == 0) vfirst_.alloc(kVfCount);
    IPO_HIP_CHECK(hipMemsetAsync(vfirst_.get(), 0x7f, kVfCount * sizeof(int), s));
    int* vf = vfirst_.get();
    launch_first_nonpositive(n, x, vf + kVfX, s);
    launch_first_nonpositive(m, y, vf + kVfY, s);
    launch_first_nonpositive(m, w, vf + kVfW, s);
    launch_first_nonpositive(n, z, vf + kVfZ, s);
    int first[kVfCount];
    IPO_HIP_CHECK(hipMemcpyAsync(first, vf, sizeof first, hipMemcpyDeviceToHost, s));
    IPO_HIP_CHECK(hipStreamSynchronize(s));
    const std::pair<int, const char*> chk[] = {{kVfX, "x"}, {kVfY, "y"}, {kVfW, "w"}, {kVfZ, "z"}};
    for (const auto& c : chk)
        if (first[c.first] != kVfNone && first[c.first] < ((c.first == kVfX || c.first == kVfZ) ? n : m))
            throw std::runtime_error(std::string("start rule mehrotra: ") + c.second + "[" + std::to_string(first[c.first]) +
                                     "] of the start point is not a finite value > 0");
    return passes;
}

void IpmSolver::set_start_rule(StartRule r) {
    if (sharded_) throw std::invalid_argument("set_start_rule: not supported on a sharded solver");
    rule_ = r;
    has_start_ = false;
}

void IpmSolver::start_point(StartRule r, double* x, double* y, double* w, double* z) {
    if (sharded_) throw std::invalid_argument("start_point: not supported on a sharded solver");
    if (r == StartRule::Default) {
        if (x) std::fill(x, x + n_, 1000.0);
        if (z) std::fill(z, z + n_, 1000.0);
        if (y) std::fill(y, y + m_, 1000.0);
        if (w) std::fill(w, w + m_, 1000.0);
        return;
    }
    alloc_start();
    // into set_start()'s staging, the factor's host-side state (eps_diag,
    // counters) put back afterwards: x_ ... and a held start stay as they are
    KktDevice& K = *kkt_;
    const KktDevice::HostState hs = K.host_state();
    K.set_epsdiag(1.0e-14);
    try {
        mehrotra_start(tx_.get(), ty_.get(), tw_.get(), tz_.get());
    } catch (...) {
        K.restore_host_state(hs);
        throw;
    }
    K.restore_host_state(hs);
    if (x) tx_.download(x, n_, stream_);
    if (y) ty_.download(y, m_, stream_);
    if (w) tw_.download(w, m_, stream_);
    if (z) tz_.download(z, n_, stream_);
    IPO_HIP_CHECK(hipStreamSynchronize(stream_));
}

void IpmSolver::update(const double* A, const double* b, const double* c, const double* f, const double* Q) {
    if (sharded_)
        throw std::invalid_argument("update: not supported on a sharded solver (a shard keeps the values it was created with)");
    if (Q && !has_q_) throw std::invalid_argument("update: Q given to a solver created without Q");
    if (f && !std::isfinite(*f)) throw std::invalid_argument("update: f is not finite");
    hipStream_t s = stream_;
    const double t0 = now_s();
    const int m = m_, n = n_;
    // 1. the arrays given, into staging; 2. validated there
    if (vfirst_.size() == 0) vfirst_.alloc(kVfCount);
    IPO_HIP_CHECK(hipMemsetAsync(vfirst_.get(), 0x7f, kVfCount * sizeof(int), s));    // kVfNone
    int* vf = vfirst_.get();
    if (A) { stA_.upload(A, nz_, s); launch_first_nonfinite(nz_, stA_.get(), vf + kVfA, s); }
    if (b) { stb_.upload(b, m, s); launch_first_nonfinite(m, stb_.get(), vf + kVfB, s); }
    if (c) { stc_.upload(c, n, s); launch_first_nonfinite(n, stc_.get(), vf + kVfC, s); }
    if (Q) {
        stQ_.upload(Q, qnz_, s);
        launch_first_nonfinite(qnz_, stQ_.get(), vf + kVfQ, s);
        launch_first_asymmetric(qnz_, stQ_.get(), qtmap_.get(), vf + kVfQsym, s);
    }
    int first[kVfCount];
    IPO_HIP_CHECK(hipMemcpyAsync(first, vf, sizeof first, hipMemcpyDeviceToHost, s));
    IPO_HIP_CHECK(hipStreamSynchronize(s));
    t_upd_upload_ = now_s() - t0;
    t_upd_refresh_ = 0.0;
    const auto refuse = [&](int slot, int len, const char* what, const char* why) {
        if (first[slot] != kVfNone && first[slot] < len)
            throw std::invalid_argument(std::string("update: ") + what + "[" + std::to_string(first[slot]) + "] " + why);
    };
    if (A) refuse(kVfA, nz_, "A", "is not finite");
    if (b) refuse(kVfB, m, "b", "is not finite");
    if (c) refuse(kVfC, n, "c", "is not finite");
    if (Q) {
        refuse(kVfQ, qnz_, "Q", "is not finite");
        refuse(kVfQsym, qnz_, "Q", "differs from its transposed entry (Q is not symmetric)");
    }
    // 3. committed: copies and gathers on the stream, nothing can refuse now
    const double t1 = now_s();
    const double* dAk = nullptr;      // A in the factor's own CSC order
    if (A) {
        if (has_q_) {                 // the factor holds A' (run_qp): its "A" is the CSR of A
            if (stAt_.size() < static_cast<size_t>(nz_)) stAt_.alloc(nz_);
            launch_gather_map(nz_, ucsr_.get(), stA_.get(), stAt_.get(), s);
            dAk = stAt_.get();
        } else {
            dAk = stA_.get();
        }
        if (axsliced_) axplan_.refresh(stA_.get(), s);
    }
    kkt_->refresh_values(dAk, Q ? stQ_.get() : nullptr);
    if (b && m) IPO_HIP_CHECK(hipMemcpyAsync(b_.get(), stb_.get(), m * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (c && n) IPO_HIP_CHECK(hipMemcpyAsync(c_.get(), stc_.get(), n * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (f) f_ = *f;
    IPO_HIP_CHECK(hipStreamSynchronize(s));
    t_upd_refresh_ = now_s() - t1;
}

void IpmSolver::alloc_start() {
    const size_t mm = m_ > 0 ? m_ : 1, nn = n_ > 0 ? n_ : 1;
    if (sx_.size()) return;
    for (DevBuf<double>* v : {&sx_, &sz_, &tx_, &tz_}) v->alloc(nn);
    for (DevBuf<double>* v : {&sy_, &sw_, &ty_, &tw_}) v->alloc(mm);
}

void IpmSolver::set_start(const double* x, const double* y, const double* w, const double* z) {
    if (sharded_) throw std::invalid_argument("set_start: not supported on a sharded solver");
    if (!x && !y && !w && !z) { has_start_ = false; rule_ = StartRule::Default; return; }
    if (!x || !y || !w || !z) throw std::invalid_argument("set_start: x, y, w and z are given together (all null clears the start)");
    hipStream_t s = stream_;
    const int m = m_, n = n_;
    alloc_start();
    if (vfirst_.size() == 0) vfirst_.alloc(kVfCount);
    IPO_HIP_CHECK(hipMemsetAsync(vfirst_.get(), 0x7f, kVfCount * sizeof(int), s));
    int* vf = vfirst_.get();
    tx_.upload(x, n, s); launch_first_nonpositive(n, tx_.get(), vf + kVfX, s);
    ty_.upload(y, m, s); launch_first_nonpositive(m, ty_.get(), vf + kVfY, s);
    tw_.upload(w, m, s); launch_first_nonpositive(m, tw_.get(), vf + kVfW, s);
    tz_.upload(z, n, s); launch_first_nonpositive(n, tz_.get(), vf + kVfZ, s);
    int first[kVfCount];
    IPO_HIP_CHECK(hipMemcpyAsync(first, vf, sizeof first, hipMemcpyDeviceToHost, s));
    IPO_HIP_CHECK(hipStreamSynchronize(s));
    const std::pair<int, const char*> chk[] = {{kVfX, "x"}, {kVfY, "y"}, {kVfW, "w"}, {kVfZ, "z"}};
    for (const auto& c : chk)
        if (first[c.first] != kVfNone && first[c.first] < ((c.first == kVfX || c.first == kVfZ) ? n : m))
            throw std::invalid_argument(std::string("set_start: ") + c.second + "[" + std::to_string(first[c.first]) +
                                        "] is not a finite value > 0");
    ClampJobs J{};       // the copy into the held start: floor 0 leaves positive values as they are
    J.src[0] = tx_.get(); J.dst[0] = sx_.get(); J.len[0] = n;
    J.src[1] = ty_.get(); J.dst[1] = sy_.get(); J.len[1] = m;
    J.src[2] = tw_.get(); J.dst[2] = sw_.get(); J.len[2] = m;
    J.src[3] = tz_.get(); J.dst[3] = sz_.get(); J.len[3] = n;
    launch_clamp_copy4(J, 0.0, s);
    IPO_HIP_CHECK(hipStreamSynchronize(s));
    has_start_ = true;
    rule_ = StartRule::Default;
}

void IpmSolver::start_from_last(double floor) {
    if (sharded_) throw std::invalid_argument("start_from_last: not supported on a sharded solver");
    if (!ran_) throw std::invalid_argument("start_from_last: no run on this solver yet");
    if (!(floor > 0.0) || !std::isfinite(floor)) throw std::invalid_argument("start_from_last: floor must be finite and > 0");
    alloc_start();
    ClampJobs J{};
    J.src[0] = x_.get(); J.dst[0] = sx_.get(); J.len[0] = n_;
    J.src[1] = y_.get(); J.dst[1] = sy_.get(); J.len[1] = m_;
    J.src[2] = w_.get(); J.dst[2] = sw_.get(); J.len[2] = m_;
    J.src[3] = z_.get(); J.dst[3] = sz_.get(); J.len[3] = n_;
    launch_clamp_copy4(J, floor, stream_);
    has_start_ = true;
    rule_ = StartRule::Default;
}

int IpmSolver::run_hsd(const IpmOptions& opt, IpmResult* res) {
    // mu, residuals and right-hand sides on a side stream beside the
    // factorisation (one GPU, no exchange); IPO_HIP_OVERLAP=0 turns it off
    const bool overlap = xch_ == nullptr && knobs_.overlap;
    const int m = m_, n = n_;
    hipStream_t s = stream_;
    const int gv = ceil_div(m + n, NT);
    FILE* tr = opt.trace;
    hipLaunchKernelGGL(k_fill, dim3(ceil_div(n, NT)), dim3(NT), 0, s, n, 1.0, x_.get());
    hipLaunchKernelGGL(k_fill, dim3(ceil_div(n, NT)), dim3(NT), 0, s, n, 1.0, z_.get());
    hipLaunchKernelGGL(k_fill, dim3(ceil_div(m, NT)), dim3(NT), 0, s, m, 1.0, w_.get());
    hipLaunchKernelGGL(k_fill, dim3(ceil_div(m, NT)), dim3(NT), 0, s, m, 1.0, y_.get());
    double phi = 1.0, psi = 1.0;
    if (tr) {
        print_dims(tr);
        std::fputs(kHsdHeader, tr);
        std::fflush(tr);
    }
    KktDevice& K = *kkt_;
    int status = 5, iter;
    // one host synchronisation per iteration outside the KKT solver: the
    // dots of mu (with phi / psi of the device step, hsd.c:264-265); the
    // residual norms are only printed (read back without a wait), dphi /
    // dpsi / theta / phi / psi are computed on the device (k_hsd_dphi,
    // k_hsd_theta: the host's operations in the host's order)
    for (iter = 0; iter < opt.max_iter; iter++) {
        RedJobs j{};
        j.nj = 4;
        j.segmin = dot_segmin_;
        j.a[0] = z_.get(); j.b[0] = x_.get(); j.len[0] = n; j.op[0] = 0;
        j.a[1] = w_.get(); j.b[1] = y_.get(); j.len[1] = mcnt_; j.op[1] = 0;
        j.a[2] = c_.get(); j.b[2] = x_.get(); j.len[2] = n; j.op[2] = 0;
        j.a[3] = b_.get(); j.b[3] = y_.get(); j.len[3] = mcnt_; j.op[3] = 0;
        const double delta = (iter % 2 == 0) ? 0.0 : 1.0;
        KktDevice::HostState spec{};
        std::exception_ptr spec_err;
        if (overlap) {
            // side stream: the dots of mu, mu, the residuals and their norms
            // (device phi / mu) beside the factorisation on the main stream
            IPO_HIP_CHECK(hipEventRecord(ev_step_, s));
            IPO_HIP_CHECK(hipStreamWaitEvent(side_, ev_step_, 0));
            launch_reduce(j, part2_.get(), scal_.get(), side_);
            hipLaunchKernelGGL(k_hsd_mu, dim3(1), dim3(1), 0, side_, scal_.get(), static_cast<double>(ng_ + mg_ + 1), phi,
                               psi, iter > 0 ? 1 : 0);
            row_ax(x_.get(), side_);
            hipLaunchKernelGGL(k_hsd_residuals, dim3(kRedBlocks), dim3(kResThreads), 0, side_, m, n, K.kAt(), K.iAt(),
                               K.At(), K.kA(), K.iA(), K.A(), b_.get(), c_.get(), x_.get(), y_.get(), w_.get(), z_.get(),
                               phi, delta, 0.0, E_.get(), D_.get(), fy_.get(), fx_.get(), gy_.get(), gx_.get(),
                               part2_.get(), mrow(), mcnt_, lax(), static_cast<const double*>(scal_.get() + kIsPhiMu));
            hipLaunchKernelGGL(k_finish_reduce, dim3(1), dim3(kRedThreads), 0, side_, part2_.get(), 2, 0u,
                               scal_.get() + kIsNorm2);
            IPO_HIP_CHECK(hipMemcpyAsync(hs_, scal_.get(), kIsCount * sizeof(double), hipMemcpyDeviceToHost, side_));
            IPO_HIP_CHECK(hipEventRecord(ev_side_, side_));
            hipLaunchKernelGGL(k_hsd_scaling, dim3(gv), dim3(NT), 0, s, m, n, x_.get(), y_.get(), w_.get(), z_.get(),
                               E_.get(), D_.get());
            // speculative: the host learns mu (and so whether hsd.c:155 stops
            // here, where the reference does not factor) only after it; its
            // host-side effects are undone and an error it raised is held
            // back unless the iteration goes on to use the factor
            spec = K.host_state();
            // the solves' right-hand sides are final at ev_side_: the factor
            // runs their forward sparse sweep on the side stream beside its
            // dense tail (KktDevice::PrePass), and solve2 below picks it up
            KktDevice::PrePass pre;
            pre.R = 2;
            pre.dfy[0] = fy_.get(); pre.dfx[0] = fx_.get();
            pre.dfy[1] = gy_.get(); pre.dfx[1] = gx_.get();
            pre.stream = side_;
            pre.ready = ev_side_;
            try {
                K.factor(E_.get(), D_.get(), &pre);
            } catch (...) {
                spec_err = std::current_exception();
            }
            IPO_HIP_CHECK(hipEventSynchronize(ev_side_));
        } else {
            launch_reduce(j, part_.get(), scal_.get(), s);
            xsum(scal_.get(), 4, RedOp::Sum);
            IPO_HIP_CHECK(hipMemcpyAsync(hs_, scal_.get(), 4 * sizeof(double), hipMemcpyDeviceToHost, s));
            if (iter > 0)
                IPO_HIP_CHECK(hipMemcpyAsync(hs_ + kIsPhiNext, scal_.get() + kIsPhiNext, 2 * sizeof(double),
                                             hipMemcpyDeviceToHost, s));
            IPO_HIP_CHECK(hipStreamSynchronize(s));
        }
        if (iter > 0) { phi = hs_[kIsPhiNext]; psi = hs_[kIsPhiNext + 1]; }
        const double mu = (hs_[kIsZx] + hs_[kIsWy] + phi * psi) / (ng_ + mg_ + 1);
        // the device's mu / phi must be the host's bit for bit (NaNs included:
        // a diverging solve then takes the sequential path's status route)
        if (overlap && (std::memcmp(&mu, &hs_[kIsPhiMu + 1], sizeof mu) != 0 ||
                        std::memcmp(&phi, &hs_[kIsPhiMu], sizeof phi) != 0))
            throw std::runtime_error("hsd: device mu / phi differ from the host's");
        const double pobj = hs_[kIsCx], dobj = hs_[kIsBy];
        if (mu < 1.0e-12) {
            if (overlap) K.restore_host_state(spec);     // the speculative factorisation is not used
            if (phi > psi) status = 0;
            else if (dobj < 0.0) status = 2;
            else if (pobj > 0.0) status = 4;
            else { if (tr) std::fprintf(tr, "Trouble in river city \n"); status = 4; }
            break;
        }
        if (!overlap) {
            link_ax(x_.get());
            hipLaunchKernelGGL(k_hsd_residuals, dim3(kRedBlocks), dim3(kResThreads), 0, s, m, n, K.kAt(), K.iAt(), K.At(),
                               K.kA(), K.iA(), K.A(), b_.get(), c_.get(), x_.get(), y_.get(), w_.get(), z_.get(), phi,
                               delta, mu, E_.get(), D_.get(), fy_.get(), fx_.get(), gy_.get(), gx_.get(), part_.get(),
                               mrow(), mcnt_, lax(), static_cast<const double*>(nullptr));
            hipLaunchKernelGGL(k_finish_reduce, dim3(1), dim3(kRedThreads), 0, s, part_.get(), 2, 0u, scal_.get());
            xsum(scal_.get(), 2, RedOp::Sum);
            IPO_HIP_CHECK(hipMemcpyAsync(hs_ + kIsNorm2, scal_.get() + kIsRed, 2 * sizeof(double),
                                         hipMemcpyDeviceToHost, s));
            K.factor(E_.get(), D_.get());    // synchronises the stream: hs_'s kIsNorm2 have landed
        } else {
            if (spec_err) std::rethrow_exception(spec_err);
            IPO_HIP_CHECK(hipStreamWaitEvent(s, ev_side_, 0));   // fy fx gy gx before the solves
        }
        const double gamma = -(1 - delta) * (dobj - pobj + psi) + psi - delta * mu / phi;

        const double normr = std::sqrt(hs_[kIsNorm2]) / phi;
        const double norms = std::sqrt(hs_[kIsNorm2 + 1]) / phi;
        if (tr) {
            std::fprintf(tr, "%8d   %14.7e  %8.1e    %14.7e  %8.1e  %8.1e \n", iter, pobj / phi + f_, normr,
                         dobj / phi + f_, norms, mu);
            std::fflush(tr);
        }
        res->final_mu = mu; res->final_pobj = pobj / phi + f_; res->final_dobj = dobj / phi + f_;
        res->final_pinf = normr; res->final_dinf = norms;
        if (knobs_.trace_full) {
            std::fprintf(stderr, "FT %d %.17g %.17g %.17g %.17g %.17g %.17g\n", iter, pobj, dobj, mu, phi, psi, normr);
            std::fprintf(stderr, "FT   ndep=%d eps=%.1e\n", K.ndep(), K.epsdiag());
        }
        // the two forwardbackward calls of hsd.c:218-224 / hsdls.c:194-203,
        // independent systems with one factor: sweeps batched
        K.solve2(E_.get(), D_.get(), fy_.get(), fx_.get(), gy_.get(), gx_.get());
        res->refine_passes += K.last_passes();

        RedJobs q{};
        q.nj = 4;
        q.segmin = dot_segmin_;
        q.a[0] = c_.get(); q.b[0] = fx_.get(); q.len[0] = n; q.op[0] = 0;
        q.a[1] = b_.get(); q.b[1] = fy_.get(); q.len[1] = mcnt_; q.op[1] = 0;
        q.a[2] = c_.get(); q.b[2] = gx_.get(); q.len[2] = n; q.op[2] = 0;
        q.a[3] = b_.get(); q.b[3] = gy_.get(); q.len[3] = mcnt_; q.op[3] = 0;
        launch_reduce(q, part_.get(), scal_.get(), s);
        xsum(scal_.get(), 4, RedOp::Sum);
        hipLaunchKernelGGL(k_hsd_dphi, dim3(1), dim3(1), 0, s, scal_.get(), gamma, delta, mu, phi, psi);
        hipLaunchKernelGGL(k_hsd_directions, dim3(kRedBlocks), dim3(NT), 0, s, m, n, scal_.get() + kIsDphi, delta, mu,
                           fx_.get(), gx_.get(), fy_.get(), gy_.get(), x_.get(), z_.get(), y_.get(), w_.get(), D_.get(),
                           E_.get(), dx_.get(), dz_.get(), dy_.get(), dw_.get(), part_.get());
        hipLaunchKernelGGL(k_finish_reduce, dim3(1), dim3(kRedThreads), 0, s, part_.get(), 1, 1u, scal_.get());
        xsum(scal_.get(), 1, RedOp::Max);
        hipLaunchKernelGGL(k_hsd_theta, dim3(1), dim3(1), 0, s, scal_.get(), phi, psi);
        hipLaunchKernelGGL(k_step, dim3(gv), dim3(NT), 0, s, m, n, 0.0, scal_.get() + kIsTheta, x_.get(), dx_.get(),
                           z_.get(), dz_.get(), y_.get(), dy_.get(), w_.get(), dw_.get());
    }
    hipLaunchKernelGGL(k_unscale, dim3(gv), dim3(NT), 0, s, m, n, phi, x_.get(), z_.get(), y_.get(), w_.get());
    IPO_HIP_CHECK(hipGetLastError());
    IPO_HIP_CHECK(hipStreamSynchronize(s));
    res->iters = iter;
    res->phi = phi;
    res->psi = psi;
    return status;
}

// hsdls.c:38-296 -- same residuals and solves as HSD with a fixed centring
// delta = 2 (1 - beta), beta = 0.8, and a quadratic linesearch for theta
int IpmSolver::run_hsdls(const IpmOptions& opt, IpmResult* res) {
    const int m = m_, n = n_;
    hipStream_t s = stream_;
    const int gv = ceil_div(m + n, NT);
    FILE* tr = opt.trace;
    hipLaunchKernelGGL(k_fill, dim3(ceil_div(n, NT)), dim3(NT), 0, s, n, 1.0, x_.get());
    hipLaunchKernelGGL(k_fill, dim3(ceil_div(n, NT)), dim3(NT), 0, s, n, 1.0, z_.get());
    hipLaunchKernelGGL(k_fill, dim3(ceil_div(m, NT)), dim3(NT), 0, s, m, 1.0, w_.get());
    hipLaunchKernelGGL(k_fill, dim3(ceil_div(m, NT)), dim3(NT), 0, s, m, 1.0, y_.get());
    double phi = 1.0, psi = 1.0;
    if (tr) {
        print_dims(tr);
        std::fputs(kHsdHeader, tr);
        std::fflush(tr);
    }
    const double beta = 0.80, delta = 2 * (1 - beta);
    KktDevice& K = *kkt_;
    int status = 5, iter;
    for (iter = 0; iter < opt.max_iter; iter++) {
        RedJobs j{};
        j.nj = 4;
        j.segmin = dot_segmin_;
        j.a[0] = z_.get(); j.b[0] = x_.get(); j.len[0] = n; j.op[0] = 0;
        j.a[1] = w_.get(); j.b[1] = y_.get(); j.len[1] = mcnt_; j.op[1] = 0;
        j.a[2] = c_.get(); j.b[2] = x_.get(); j.len[2] = n; j.op[2] = 0;
        j.a[3] = b_.get(); j.b[3] = y_.get(); j.len[3] = mcnt_; j.op[3] = 0;
        reduce(j, 4);
        const double mu = (hs_[kIsZx] + hs_[kIsWy] + phi * psi) / (ng_ + mg_ + 1);
        const double pobj = hs_[kIsCx], dobj = hs_[kIsBy];
        if (mu < 1.0e-12) {                                   // hsdls.c:131-153
            if (phi > 1.0e-12) status = 0;
            else if (dobj < 0.0) status = 2;
            else if (pobj > 0.0) status = 4;
            else status = 7;
            break;
        }
        link_ax(x_.get());
        hipLaunchKernelGGL(k_hsd_residuals, dim3(kRedBlocks), dim3(kResThreads), 0, s, m, n, K.kAt(), K.iAt(), K.At(), K.kA(),
                           K.iA(), K.A(), b_.get(), c_.get(), x_.get(), y_.get(), w_.get(), z_.get(), phi, delta, mu,
                           E_.get(), D_.get(), fy_.get(), fx_.get(), gy_.get(), gx_.get(), part_.get(), mrow(), mcnt_,
                           lax(), static_cast<const double*>(nullptr));
        hipLaunchKernelGGL(k_finish_reduce, dim3(1), dim3(kRedThreads), 0, s, part_.get(), 2, 0u, scal_.get());
        xsum(scal_.get(), 2, RedOp::Sum);
        IPO_HIP_CHECK(hipMemcpyAsync(hs_, scal_.get(), 2 * sizeof(double), hipMemcpyDeviceToHost, s));
        IPO_HIP_CHECK(hipStreamSynchronize(s));
        const double normr = std::sqrt(hs_[kIsRed]) / phi;
        const double norms = std::sqrt(hs_[kIsRed + 1]) / phi;
        const double gamma = -(1 - delta) * (dobj - pobj + psi) + psi - delta * mu / phi;
        if (tr) {
            std::fprintf(tr, "%8d   %14.7e  %8.1e    %14.7e  %8.1e  %8.1e \n", iter, pobj / phi + f_, normr,
                         dobj / phi + f_, norms, mu);
            std::fflush(tr);
        }
        res->final_mu = mu; res->final_pobj = pobj / phi + f_; res->final_dobj = dobj / phi + f_;
        res->final_pinf = normr; res->final_dinf = norms;

        K.factor(E_.get(), D_.get());
        // the two forwardbackward calls of hsd.c:218-224 / hsdls.c:194-203,
        // independent systems with one factor: sweeps batched
        K.solve2(E_.get(), D_.get(), fy_.get(), fx_.get(), gy_.get(), gx_.get());
        res->refine_passes += K.last_passes();

        RedJobs q{};
        q.nj = 4;
        q.segmin = dot_segmin_;
        q.a[0] = c_.get(); q.b[0] = fx_.get(); q.len[0] = n; q.op[0] = 0;
        q.a[1] = b_.get(); q.b[1] = fy_.get(); q.len[1] = mcnt_; q.op[1] = 0;
        q.a[2] = c_.get(); q.b[2] = gx_.get(); q.len[2] = n; q.op[2] = 0;
        q.a[3] = b_.get(); q.b[3] = gy_.get(); q.len[3] = mcnt_; q.op[3] = 0;
        reduce(q, 4);
        const double dphi = (hs_[kIsRed] - hs_[kIsRed + 1] + gamma) / (hs_[kIsRed + 2] - hs_[kIsRed + 3] - psi / phi);
        const double dpsi = delta * mu / phi - psi - (psi / phi) * dphi;

        hipLaunchKernelGGL(k_hsdls_directions, dim3(kRedBlocks), dim3(NT), 0, s, m, n, dphi, beta, delta, mu, fx_.get(),
                           gx_.get(), fy_.get(), gy_.get(), x_.get(), z_.get(), y_.get(), w_.get(), D_.get(), E_.get(),
                           dx_.get(), dz_.get(), dy_.get(), dw_.get(), part_.get());
        hipLaunchKernelGGL(k_finish_reduce, dim3(1), dim3(kRedThreads), 0, s, part_.get(), 1, 1u, scal_.get());
        xsum(scal_.get(), 1, RedOp::Max);
        IPO_HIP_CHECK(hipMemcpyAsync(hs_, scal_.get(), sizeof(double), hipMemcpyDeviceToHost, s));
        IPO_HIP_CHECK(hipStreamSynchronize(s));
        double theta = 1.0;
        const double tv = -hs_[kIsRed];       // min over the vector entries
        theta = theta < tv ? theta : tv;
        const double tp = ls_step_host(phi, psi, dphi, dpsi, beta, delta, mu);
        theta = theta < tp ? theta : tp;
        if (theta < 1.0) theta *= 0.9999;

        hipLaunchKernelGGL(k_step, dim3(gv), dim3(NT), 0, s, m, n, theta, static_cast<const double*>(nullptr), x_.get(), dx_.get(), z_.get(), dz_.get(),
                           y_.get(), dy_.get(), w_.get(), dw_.get());
        phi = phi + theta * dphi;
        psi = psi + theta * dpsi;
    }
    hipLaunchKernelGGL(k_unscale, dim3(gv), dim3(NT), 0, s, m, n, phi, x_.get(), z_.get(), y_.get(), w_.get());
    IPO_HIP_CHECK(hipGetLastError());
    IPO_HIP_CHECK(hipStreamSynchronize(s));
    res->iters = iter;
    res->phi = phi;
    res->psi = psi;
    return status;
}

int IpmSolver::run_intpt(const IpmOptions& opt, IpmResult* res) {
    const int m = m_, n = n_;
    hipStream_t s = stream_;
    const int gv = ceil_div(m + n, NT);
    FILE* tr = opt.trace;
    init_point(1000.0, res);
    const double delta = 0.02, r = 0.9;
    double normr0 = HUGE_VAL, norms0 = HUGE_VAL;
    if (tr) {
        print_dims(tr);
        std::fputs(kIntptHeader, tr);
        std::fflush(tr);
    }
    KktDevice& K = *kkt_;
    int status = 5, iter;
    for (iter = 0; iter < opt.max_iter; iter++) {
        link_ax(x_.get());
        hipLaunchKernelGGL(k_pf_residuals, dim3(kRedBlocks), dim3(kResThreads), 0, s, m, n, K.kAt(), K.iAt(), K.At(), K.kA(),
                           K.iA(), K.A(), b_.get(), c_.get(), x_.get(), y_.get(), w_.get(), z_.get(), rho_.get(),
                           sig_.get(), part_.get(), mrow(), mcnt_, lax());
        hipLaunchKernelGGL(k_finish_reduce, dim3(1), dim3(kRedThreads), 0, s, part_.get(), 2, 0u, scal_.get() + kIsNorm2);
        RedJobs j{};
        j.nj = 4;
        j.segmin = dot_segmin_;
        j.a[0] = z_.get(); j.b[0] = x_.get(); j.len[0] = n; j.op[0] = 0;
        j.a[1] = y_.get(); j.b[1] = w_.get(); j.len[1] = mcnt_; j.op[1] = 0;
        j.a[2] = c_.get(); j.b[2] = x_.get(); j.len[2] = n; j.op[2] = 0;
        j.a[3] = b_.get(); j.b[3] = y_.get(); j.len[3] = mcnt_; j.op[3] = 0;
        launch_reduce(j, part_.get(), scal_.get(), s);
        xsum(scal_.get(), 4, RedOp::Sum);
        xsum(scal_.get() + kIsNorm2, 2, RedOp::Sum);
        IPO_HIP_CHECK(hipMemcpyAsync(hs_, scal_.get(), (kIsNorm2 + 2) * sizeof(double), hipMemcpyDeviceToHost, s));
        IPO_HIP_CHECK(hipStreamSynchronize(s));
        // intpt.c:47 keeps the printed quantities in single precision
        const float normr = static_cast<float>(std::sqrt(hs_[kIsNorm2]));
        const float norms = static_cast<float>(std::sqrt(hs_[kIsNorm2 + 1]));
        const double gamma = hs_[kIsZx] + hs_[kIsWy];
        const float pobj = static_cast<float>(hs_[kIsCx] + f_);
        const float dobj = static_cast<float>(hs_[kIsBy] + f_);
        if (tr) {
            std::fprintf(tr, "%8d   %14.7e  %8.1e    %14.7e  %8.1e \n", iter, pobj, normr, dobj, norms);
            std::fflush(tr);
        }
        res->final_mu = gamma; res->final_pobj = pobj; res->final_dobj = dobj;
        res->final_pinf = normr; res->final_dinf = norms;
        if (normr < 1.0e-6 && norms < 1.0e-6 && gamma < 1.0e-6) { status = 0; break; }
        if (normr > 10 * normr0) { status = 2; break; }
        if (norms > 10 * norms0) { status = 4; break; }
        const double mu = delta * gamma / (ng_ + mg_);
        hipLaunchKernelGGL(k_pf_rhs, dim3(gv), dim3(NT), 0, s, m, n, mu, x_.get(), z_.get(), y_.get(), w_.get(),
                           rho_.get(), sig_.get(), D_.get(), E_.get(), dx_.get(), dy_.get());
        K.factor(E_.get(), D_.get());
        K.solve(E_.get(), D_.get(), dy_.get(), dx_.get());
        res->refine_passes += K.last_passes();
        hipLaunchKernelGGL(k_pf_directions, dim3(kRedBlocks), dim3(NT), 0, s, m, n, mu, x_.get(), z_.get(), y_.get(),
                           w_.get(), D_.get(), E_.get(), dx_.get(), dy_.get(), dz_.get(), dw_.get(), part_.get());
        hipLaunchKernelGGL(k_finish_reduce, dim3(1), dim3(kRedThreads), 0, s, part_.get(), 1, 1u, scal_.get());
        xsum(scal_.get(), 1, RedOp::Max);
        IPO_HIP_CHECK(hipMemcpyAsync(hs_, scal_.get(), sizeof(double), hipMemcpyDeviceToHost, s));
        IPO_HIP_CHECK(hipStreamSynchronize(s));
        double theta = hs_[kIsRed];
        theta = (r / theta > 1.0) ? 1.0 : r / theta;
        hipLaunchKernelGGL(k_step, dim3(gv), dim3(NT), 0, s, m, n, theta, static_cast<const double*>(nullptr), x_.get(), dx_.get(), z_.get(), dz_.get(),
                           y_.get(), dy_.get(), w_.get(), dw_.get());
        normr0 = normr;
        norms0 = norms;
    }
    IPO_HIP_CHECK(hipGetLastError());
    IPO_HIP_CHECK(hipStreamSynchronize(s));
    res->iters = iter;
    return status;
}

// run_intpt with a quadratic objective term, max c'x + f - x'Qx / 2 (an
// extension: the reference has no QP loop).  Same start, delta, r, stopping
// and give-up tests, printed quantities and trace as run_intpt; sigma and
// the objectives carry Q (k_qp_residuals), and the Newton system is
//   -E dy + A dx = rho + w - mu / y,   A'dy + (D + Q) dx = sigma - z + mu / x.
// The solver holds the factor of the swapped roles (KktDevice on A' with
// E' = D, D' = E and Q on its first block), called with fy' = -fx,
// fx' = fy and read back as dx = dy', dy = -dx' (k_qp_rhs, k_qp_directions);
// its kA() is the CSR of A and its kAt() the CSC.  (Without Q the problem is
// the LP and run() takes run_intpt.)
int IpmSolver::run_qp(const IpmOptions& opt, IpmResult* res) {
    const int m = m_, n = n_;
    hipStream_t s = stream_;
    const int gv = ceil_div(m + n, NT);
    FILE* tr = opt.trace;
    init_point(1000.0, res);
    const double delta = 0.02, r = 0.9;
    double normr0 = HUGE_VAL, norms0 = HUGE_VAL;
    if (tr) {
        print_dims(tr);
        std::fputs(kIntptHeader, tr);
        std::fflush(tr);
    }
    KktDevice& K = *kkt_;
    int status = 5, iter;
    for (iter = 0; iter < opt.max_iter; iter++) {
        row_ax(x_.get(), s);
        if (K.q_long_count() > 0) K.launch_q_long(x_.get(), qx_.get());     // Q's long columns, one wave each
        hipLaunchKernelGGL(k_qp_residuals, dim3(kRedBlocks), dim3(kResThreads), 0, s, m, n, K.kA(), K.iA(), K.A(), K.kAt(),
                           K.iAt(), K.At(), K.kQ(), K.iQ(), K.Q(), b_.get(), c_.get(), x_.get(), y_.get(), w_.get(), z_.get(), rho_.get(),
                           sig_.get(), qx_.get(), part_.get(), mrow(), lax(), K.q_long_min());
        hipLaunchKernelGGL(k_finish_reduce, dim3(1), dim3(kRedThreads), 0, s, part_.get(), 2, 0u, scal_.get() + kIsNorm2);
        RedJobs j{};
        j.nj = 5;
        j.segmin = dot_segmin_;
        j.a[0] = z_.get(); j.b[0] = x_.get(); j.len[0] = n; j.op[0] = 0;
        j.a[1] = y_.get(); j.b[1] = w_.get(); j.len[1] = m; j.op[1] = 0;
        j.a[2] = c_.get(); j.b[2] = x_.get(); j.len[2] = n; j.op[2] = 0;
        j.a[3] = b_.get(); j.b[3] = y_.get(); j.len[3] = m; j.op[3] = 0;
        j.a[4] = x_.get(); j.b[4] = qx_.get(); j.len[4] = n; j.op[4] = 0;     // x'Qx
        launch_reduce(j, part_.get(), scal_.get(), s);
        IPO_HIP_CHECK(hipMemcpyAsync(hs_, scal_.get(), (kIsNorm2 + 2) * sizeof(double), hipMemcpyDeviceToHost, s));
        IPO_HIP_CHECK(hipStreamSynchronize(s));
        // the printed quantities in single precision, as run_intpt (intpt.c:47)
        const float normr = static_cast<float>(std::sqrt(hs_[kIsNorm2]));
        const float norms = static_cast<float>(std::sqrt(hs_[kIsNorm2 + 1]));
        const double gamma = hs_[kIsZx] + hs_[kIsWy];
        const double hxqx = 0.5 * hs_[kIsXqx];
        const float pobj = static_cast<float>(hs_[kIsCx] - hxqx + f_);
        const float dobj = static_cast<float>(hs_[kIsBy] + hxqx + f_);
        if (tr) {
            std::fprintf(tr, "%8d   %14.7e  %8.1e    %14.7e  %8.1e \n", iter, pobj, normr, dobj, norms);
            std::fflush(tr);
        }
        res->final_mu = gamma; res->final_pobj = pobj; res->final_dobj = dobj;
        res->final_pinf = normr; res->final_dinf = norms;
        if (normr < 1.0e-6 && norms < 1.0e-6 && gamma < 1.0e-6) { status = 0; break; }
        if (normr > 10 * normr0) { status = 2; break; }
        if (norms > 10 * norms0) { status = 4; break; }
        const double mu = delta * gamma / (n + m);
        hipLaunchKernelGGL(k_qp_rhs, dim3(gv), dim3(NT), 0, s, m, n, mu, x_.get(), z_.get(), y_.get(), w_.get(),
                           rho_.get(), sig_.get(), D_.get(), E_.get(), dx_.get(), dy_.get());
        K.factor(D_.get(), E_.get());
        K.solve(D_.get(), E_.get(), dx_.get(), dy_.get());
        res->refine_passes += K.last_passes();
        hipLaunchKernelGGL(k_qp_directions, dim3(kRedBlocks), dim3(NT), 0, s, m, n, mu, x_.get(), z_.get(), y_.get(),
                           w_.get(), D_.get(), E_.get(), dx_.get(), dy_.get(), dz_.get(), dw_.get(), part_.get());
        hipLaunchKernelGGL(k_finish_reduce, dim3(1), dim3(kRedThreads), 0, s, part_.get(), 1, 1u, scal_.get());
        IPO_HIP_CHECK(hipMemcpyAsync(hs_, scal_.get(), sizeof(double), hipMemcpyDeviceToHost, s));
        IPO_HIP_CHECK(hipStreamSynchronize(s));
        double theta = hs_[kIsRed];
        theta = (r / theta > 1.0) ? 1.0 : r / theta;
        hipLaunchKernelGGL(k_step, dim3(gv), dim3(NT), 0, s, m, n, theta, static_cast<const double*>(nullptr), x_.get(), dx_.get(), z_.get(), dz_.get(),
                           y_.get(), dy_.get(), w_.get(), dw_.get());
        normr0 = normr;
        norms0 = norms;
    }
    IPO_HIP_CHECK(hipGetLastError());
    IPO_HIP_CHECK(hipStreamSynchronize(s));
    res->iters = iter;
    return status;
}

// Mehrotra's predictor-corrector for the problems of run_intpt (SW false: no
// Q, the LP's factor) and run_qp (SW true: the swapped factor, its calling
// convention as there); an extension, DESIGN.md §10.2.  Each iteration opens
// as theirs: the same start, residuals, gamma, objectives, printed line and
// stop rule.  The give-up tests also ask that the residual stand above
// 1e-6 (1 + its norm on line 0): a residual at its rounding floor grows
// tenfold on noise.  Then one factorisation and two refined solves:
//   predictor  right-hand sides rho + w, sigma - z; dza = -z - D dxa,
//              dwa = -w - E dya; t = the largest ratio (k_pc_affine)
//   centring   mu on the device from t, gamma and six dots (k_pc_mu)
//   corrector  right-hand sides rho + w - cy / y, sigma - z + cx / x with
//              cx = mu - dxa dza, cy = mu - dya dwa; dz = cx / x - z - D dx,
//              dw = cy / y - w - E dy; theta = min(1, 0.95 / t) (k_pc_theta)
// The predictor's dxa, dya live in gx_, gy_ (solved in place) and dza, dwa in
// fx_, fy_, so they survive the second solve in dx_, dy_.  One host
// synchronisation an iteration outside the KKT solver, the opening one: the
// predictor's scalars, mu and theta never leave the device.
template <bool SW>
int IpmSolver::run_pc(const IpmOptions& opt, IpmResult* res) {
    const int m = m_, n = n_;
    hipStream_t s = stream_;
    const int gv = ceil_div(m + n, NT);
    FILE* tr = opt.trace;
    init_point(1000.0, res);
    double normr0 = HUGE_VAL, norms0 = HUGE_VAL, normr1 = 0.0, norms1 = 0.0;
    if (tr) {
        print_dims(tr);
        std::fputs(kIntptHeader, tr);
        std::fflush(tr);
    }
    KktDevice& K = *kkt_;
    double* sc = scal_.get();
    const double* mup = sc + kIsPcMu;
    const double* nomu = nullptr;
    int status = 5, iter;
    for (iter = 0; iter < opt.max_iter; iter++) {
        row_ax(x_.get(), s);
        if (SW) {
            if (K.q_long_count() > 0) K.launch_q_long(x_.get(), qx_.get());     // Q's long columns, one wave each
            hipLaunchKernelGGL(k_qp_residuals, dim3(kRedBlocks), dim3(kResThreads), 0, s, m, n, K.kA(), K.iA(), K.A(),
                               K.kAt(), K.iAt(), K.At(), K.kQ(), K.iQ(), K.Q(), b_.get(), c_.get(), x_.get(), y_.get(),
                               w_.get(), z_.get(), rho_.get(), sig_.get(), qx_.get(), part_.get(), mrow(), lax(),
                               K.q_long_min());
        } else {
            hipLaunchKernelGGL(k_pf_residuals, dim3(kRedBlocks), dim3(kResThreads), 0, s, m, n, K.kAt(), K.iAt(), K.At(),
                               K.kA(), K.iA(), K.A(), b_.get(), c_.get(), x_.get(), y_.get(), w_.get(), z_.get(),
                               rho_.get(), sig_.get(), part_.get(), mrow(), mcnt_, lax());
        }
        hipLaunchKernelGGL(k_finish_reduce, dim3(1), dim3(kRedThreads), 0, s, part_.get(), 2, 0u, sc + kIsNorm2);
        RedJobs j{};
        j.nj = SW ? 5 : 4;
        j.segmin = dot_segmin_;
        j.a[0] = z_.get(); j.b[0] = x_.get(); j.len[0] = n; j.op[0] = 0;
        j.a[1] = y_.get(); j.b[1] = w_.get(); j.len[1] = m; j.op[1] = 0;
        j.a[2] = c_.get(); j.b[2] = x_.get(); j.len[2] = n; j.op[2] = 0;
        j.a[3] = b_.get(); j.b[3] = y_.get(); j.len[3] = m; j.op[3] = 0;
        j.a[4] = x_.get(); j.b[4] = qx_.get(); j.len[4] = n; j.op[4] = 0;     // x'Qx (SW)
        launch_reduce(j, part_.get(), sc, s);
        IPO_HIP_CHECK(hipMemcpyAsync(hs_, sc, (kIsNorm2 + 2) * sizeof(double), hipMemcpyDeviceToHost, s));
        IPO_HIP_CHECK(hipStreamSynchronize(s));
        // the printed quantities in single precision, as run_intpt (intpt.c:47)
        const float normr = static_cast<float>(std::sqrt(hs_[kIsNorm2]));
        const float norms = static_cast<float>(std::sqrt(hs_[kIsNorm2 + 1]));
        const double gamma = hs_[kIsZx] + hs_[kIsWy];
        const double hxqx = SW ? 0.5 * hs_[kIsXqx] : 0.0;
        const float pobj = static_cast<float>(hs_[kIsCx] - hxqx + f_);
        const float dobj = static_cast<float>(hs_[kIsBy] + hxqx + f_);
        if (tr) {
            std::fprintf(tr, "%8d   %14.7e  %8.1e    %14.7e  %8.1e \n", iter, pobj, normr, dobj, norms);
            std::fflush(tr);
        }
        res->final_mu = gamma; res->final_pobj = pobj; res->final_dobj = dobj;
        res->final_pinf = normr; res->final_dinf = norms;
        if (iter == 0) { normr1 = normr; norms1 = norms; }
        if (normr < 1.0e-6 && norms < 1.0e-6 && gamma < 1.0e-6) { status = 0; break; }
        if (normr > 10 * normr0 && normr >= 1.0e-6 * (1.0 + normr1)) { status = 2; break; }
        if (norms > 10 * norms0 && norms >= 1.0e-6 * (1.0 + norms1)) { status = 4; break; }
        // the predictor: dxa in gx_, dya in gy_
        hipLaunchKernelGGL(k_pc_rhs<SW>, dim3(gv), dim3(NT), 0, s, m, n, nomu, x_.get(), z_.get(), y_.get(), w_.get(),
                           rho_.get(), sig_.get(), D_.get(), E_.get(), nomu, nomu, nomu, nomu, gx_.get(), gy_.get());
        if (SW) {
            K.factor(D_.get(), E_.get());
            K.solve(D_.get(), E_.get(), gx_.get(), gy_.get());
        } else {
            K.factor(E_.get(), D_.get());
            K.solve(E_.get(), D_.get(), gy_.get(), gx_.get());
        }
        res->refine_passes += K.last_passes();
        hipLaunchKernelGGL(k_pc_affine<SW>, dim3(kRedBlocks), dim3(NT), 0, s, m, n, x_.get(), z_.get(), y_.get(), w_.get(),
                           D_.get(), E_.get(), gx_.get(), gy_.get(), fx_.get(), fy_.get(), part_.get());
        hipLaunchKernelGGL(k_finish_reduce, dim3(1), dim3(kRedThreads), 0, s, part_.get(), 1, 1u, sc + kIsPcRatio);
        RedJobs g{};
        g.nj = 6;
        g.segmin = dot_segmin_;
        g.a[0] = z_.get(); g.b[0] = gx_.get(); g.len[0] = n; g.op[0] = 0;
        g.a[1] = x_.get(); g.b[1] = fx_.get(); g.len[1] = n; g.op[1] = 0;
        g.a[2] = w_.get(); g.b[2] = gy_.get(); g.len[2] = m; g.op[2] = 0;
        g.a[3] = y_.get(); g.b[3] = fy_.get(); g.len[3] = m; g.op[3] = 0;
        g.a[4] = gx_.get(); g.b[4] = fx_.get(); g.len[4] = n; g.op[4] = 0;
        g.a[5] = gy_.get(); g.b[5] = fy_.get(); g.len[5] = m; g.op[5] = 0;
        launch_reduce(g, part_.get(), sc + kIsPcDots, s);
        hipLaunchKernelGGL(k_pc_mu, dim3(1), dim3(1), 0, s, sc, static_cast<double>(n + m));
        // the corrector, with the same factor: dx in dx_, dy in dy_
        hipLaunchKernelGGL(k_pc_rhs<SW>, dim3(gv), dim3(NT), 0, s, m, n, mup, x_.get(), z_.get(), y_.get(), w_.get(),
                           rho_.get(), sig_.get(), D_.get(), E_.get(), gx_.get(), fx_.get(), gy_.get(), fy_.get(),
                           dx_.get(), dy_.get());
        if (SW) K.solve(D_.get(), E_.get(), dx_.get(), dy_.get());
        else K.solve(E_.get(), D_.get(), dy_.get(), dx_.get());
        res->refine_passes += K.last_passes();
        hipLaunchKernelGGL(k_pc_directions<SW>, dim3(kRedBlocks), dim3(NT), 0, s, m, n, mup, x_.get(), z_.get(), y_.get(),
                           w_.get(), D_.get(), E_.get(), gx_.get(), fx_.get(), gy_.get(), fy_.get(), dx_.get(), dy_.get(),
                           dz_.get(), dw_.get(), part_.get());
        hipLaunchKernelGGL(k_finish_reduce, dim3(1), dim3(kRedThreads), 0, s, part_.get(), 1, 1u, sc);
        hipLaunchKernelGGL(k_pc_theta, dim3(1), dim3(1), 0, s, sc);
        hipLaunchKernelGGL(k_step, dim3(gv), dim3(NT), 0, s, m, n, 0.0, static_cast<const double*>(sc + kIsTheta), x_.get(),
                           dx_.get(), z_.get(), dz_.get(), y_.get(), dy_.get(), w_.get(), dw_.get());
        normr0 = normr;
        norms0 = norms;
    }
    IPO_HIP_CHECK(hipGetLastError());
    IPO_HIP_CHECK(hipStreamSynchronize(s));
    res->iters = iter;
    return status;
}

// The HBM-bound per-iteration kernels of the HSD loop timed on their own
// (bench.py's hbm_roofline leg, BASELINE configs[3] uniform): A x / A' y
// with the residual and right-hand-side vectors (k_hsd_residuals), the
// directions + ratio test (k_hsd_directions) and the step (k_step), each
// with the launch geometry of run_hsd, on device-resident inputs, `reps`
// launches timed with HIP events on one stream.  out[3] = average ms per
// launch; bytes[3] = algorithmic HBM bytes per launch (every array element
// read or written once).
void vector_bench(int m, int n, const int* kA, const int* iA, const double* A, int reps, double* out, double* bytes) {
    const long nz = kA[n];
    // CSR of A (the reference's atnum, hsd.c:111)
    std::vector<int> kAt(m + 1, 0), iAt(nz);
    std::vector<double> At(nz);
    for (long k = 0; k < nz; k++) kAt[iA[k] + 1]++;
    for (int i = 0; i < m; i++) kAt[i + 1] += kAt[i];
    {
        std::vector<int> pos(kAt.begin(), kAt.end() - 1);
        for (int j = 0; j < n; j++)
            for (int k = kA[j]; k < kA[j + 1]; k++) { iAt[pos[iA[k]]] = j; At[pos[iA[k]]++] = A[k]; }
    }
    hipStream_t s;
    IPO_HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    DevBuf<int> dkA, diA, dkAt, diAt;
    DevBuf<double> dA, dAt, vec;
    dkA.upload(kA, n + 1, s);
    diA.upload(iA, nz, s);
    dA.upload(A, nz, s);
    dkAt.upload(kAt, s);
    diAt.upload(iAt, s);
    dAt.upload(At, s);
    const size_t N = static_cast<size_t>(m) + n;
    vec.alloc(24 * N + 2 * kRedBlocks);
    {
        std::vector<double> v(24 * N, 1.0);
        for (size_t i = 0; i < v.size(); i++) v[i] = 0.5 + (i % 997) * 1e-3;
        vec.upload(v, s);
    }
    double* V = vec.get();
    auto col = [&](int q) { return V + q * N; };      // n-vectors at col(q), m-vectors at col(q) + n
    double* part = V + 24 * N;
    DevBuf<double> dphi03;
    dphi03.upload(std::vector<double>{0.3}, s);
    hipEvent_t e0, e1;
    IPO_HIP_CHECK(hipEventCreate(&e0));
    IPO_HIP_CHECK(hipEventCreate(&e1));
    const int gv = static_cast<int>((N + NT - 1) / NT);
    // the residuals as run_hsd forms them: A x column-blocked first when x
    // exceeds one L2 slice (IpmSolver::row_ax), timed together
    const KktKnobs knobs = KktKnobs::from_env();
    const int axb = knobs.ax_blocks;
    const bool sliced = rows_ax_sliced(knobs, n);
    DevBuf<double> axv;
    RowAxPlan axplan;
    if (sliced) { axv.alloc(m > 0 ? m : 1); axplan.build(m, n, kA, iA, A, axb, s); }
    for (int kq = 0; kq < 3; kq++) {
        for (int r = -2; r < reps; r++) {                 // two untimed launches first
            if (r == 0) IPO_HIP_CHECK(hipEventRecord(e0, s));
            if (kq == 0) {
                if (sliced) axplan.launch(col(2), axv.get(), s);
                hipLaunchKernelGGL(k_hsd_residuals, dim3(kRedBlocks), dim3(kResThreads), 0, s, m, n, dkAt.get(), diAt.get(),
                                   dAt.get(), dkA.get(), diA.get(), dA.get(), col(0) + n, col(1), col(2), col(3) + n,
                                   col(4) + n, col(5), 1.0, 0.5, 0.1, col(6) + n, col(7), col(8) + n, col(9),
                                   col(10) + n, col(11), part, sliced ? 0 : m, m,
                                   sliced ? static_cast<const double*>(axv.get()) : static_cast<const double*>(nullptr),
                                   static_cast<const double*>(nullptr));
            }
            else if (kq == 1)
                hipLaunchKernelGGL(k_hsd_directions, dim3(kRedBlocks), dim3(NT), 0, s, m, n, dphi03.get(), 0.5, 0.1, col(9),
                                   col(11), col(8) + n, col(10) + n, col(2), col(5), col(3) + n, col(4) + n, col(7),
                                   col(6) + n, col(12), col(13), col(14) + n, col(15) + n, part);
            else
                hipLaunchKernelGGL(k_step, dim3(gv), dim3(NT), 0, s, m, n, 1e-9, static_cast<const double*>(nullptr), col(16), col(12), col(17), col(13),
                                   col(18) + n, col(14) + n, col(19) + n, col(15) + n);
        }
        IPO_HIP_CHECK(hipEventRecord(e1, s));
        IPO_HIP_CHECK(hipEventSynchronize(e1));
        float ms = 0;
        IPO_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
        out[kq] = ms / reps;
    }
    IPO_HIP_CHECK(hipGetLastError());
    // algorithmic bytes (N = m + n): residuals -- CSR + CSC of A (12 B per
    // entry each, 4 B per pointer), b w y / c z x read once (x, y also the
    // gathered operands), E fy gy / D fx gx written: 24 nz + 4 N + 48 N;
    // directions -- 5 vectors read per row / column, 2 written: 56 N;
    // step -- 4 read, 2 written: 48 N
    bytes[0] = 24.0 * nz + 52.0 * N;
    bytes[1] = 56.0 * N;
    bytes[2] = 48.0 * N;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    IPO_HIP_CHECK(hipStreamSynchronize(s));
    (void)hipStreamDestroy(s);
}

int ipm_solve_host(int m, int n, int nz, const int* iA, const int* kA, const double* A, const double* b,
                   const double* c, double f, double* x, double* y, double* w, double* z, const IpmOptions& opt,
                   IpmResult* res) {
    (void)nz;
    IpmSolver S(m, n, kA, iA, A, b, c, f);
    const int st = S.run(opt, res);
    S.download(x, y, w, z);
    return st;
}

}  // namespace ipo
