/*
 * prisim_gains.h -- instrument gain tables on the GPU (libprisim_hip.so, prisim_amd/csrc_gains/).
 *
 * prisim/interferometry.py:GainInfo evaluates its gain tables per (label, channel, time) with FITPACK B-splines (spline_gains) or by
 * nearest neighbour (nearest_gains), and InterferometerArray.add_noise applies them: vis = gains * skyvis + noise, where the gain of the
 * baseline (A2, A1) is conj(g[A1]) g[A2] g_bl.  The entries below hold a gain table on the device in the HBM layout of the visibility
 * cube, [nt][nrows][nchan] complex128, and apply up to two such tables to a visibility cube [nt][nbl][nchan] without forming a gain cube.
 * Conventions as in prisim_hip.h: C-contiguous caller-owned host arrays, complex arrays interleaved (re, im), 0 or a negative PRISIM_E*
 * code, the message from prisim_hip_last_error().  Tables belong to the context they were made on and must be freed before it.
 */
#ifndef PRISIM_GAINS_H
#define PRISIM_GAINS_H

#include <stdint.h>

#include "prisim_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* highest spline degree the evaluation takes (FITPACK allows 1 to 5; 0 stands for an axis the table does not vary along) */
#define PRISIM_GAINS_MAX_DEGREE 5

/* factor modes of prisim_gains_apply */
enum {
  PRISIM_GAINS_ANTENNA = 0,     /* conj(g[a[b]]) * g[c[b]]: a = row of A1, c = row of A2; unity when a[b] < 0 */
  PRISIM_GAINS_BASELINE = 1     /* g[a[b]], conjugated when c[b] != 0; unity when a[b] < 0 */
};

typedef struct prisim_gains_table prisim_gains_table;

typedef struct prisim_gains_stats {
  double device_ms;       /* the call's device work, uploads and downloads included (events on the context stream) */
  double kernel_ms;       /* the kernels alone */
  int64_t elements;       /* output elements written */
} prisim_gains_stats;

/* B-spline evaluation of nrows complex rows, each two splines (real part, imaginary part) of two variables: x = time, y = frequency,
 * value(x, y) = sum_i sum_j c[(lx + i) * ncy + ly + j] * Bx_i(x) * By_j(y) (FITPACK fpbisp; splev when one axis has degree 0).
 * Spline s = 2 * row + part (part 0: real, 1: imaginary) has nx[s] knots tx at knots + kx_off[s], ny[s] knots ty at knots + ky_off[s] and
 * (nx[s] - kx - 1) * (ny[s] - ky - 1) coefficients at coefs + c_off[s].  Degrees kx, ky in 0..PRISIM_GAINS_MAX_DEGREE; nx >= 2 kx + 2,
 * ny >= 2 ky + 2.  Points outside [t[k], t[n - k - 1]] are clamped to it, as fpbisp does.  times [nt], freqs [nchan].
 * On success *out holds a new table of nt * nrows * nchan values. */
int prisim_gains_eval_spline(prisim_ctx* ctx, int64_t nrows, int32_t kx, int32_t ky, const int64_t* nx, const int64_t* ny,
                             const int64_t* kx_off, const int64_t* ky_off, const int64_t* c_off, int64_t nknots, const double* knots,
                             int64_t ncoefs, const double* coefs, int64_t nt, const double* times, int64_t nchan, const double* freqs,
                             prisim_gains_table** out, prisim_gains_stats* stats);

/* Nearest-neighbour gather: table[t][r][f] = gains[r][fidx[f]][tidx[t]] from host gains [nrows][ngf][ngt] complex128.
 * fidx [nchan] in [0, ngf), tidx [nt] in [0, ngt). */
int prisim_gains_gather(prisim_ctx* ctx, int64_t nrows, int64_t ngf, int64_t ngt, const double* gains, int64_t nchan, const int64_t* fidx,
                        int64_t nt, const int64_t* tidx, prisim_gains_table** out, prisim_gains_stats* stats);

/* shape of a table */
int prisim_gains_table_shape(const prisim_gains_table* tab, int64_t* nt, int64_t* nrows, int64_t* nchan);

/* copy a table to the host: out [nt][nrows][nchan] complex128 */
int prisim_gains_table_get(prisim_ctx* ctx, const prisim_gains_table* tab, double* out);

void prisim_gains_table_free(prisim_gains_table* tab);

/* vis[t][b][f] = g(t, b, f) * sky[t][b][f] + noise[t][b][f] for nt * nbl * nchan elements, with the gain g the product of up to two
 * factors (NULL table: absent; both absent: unity):
 *   factor(t, b, f) = mode ANTENNA:  a[b] < 0 ? 1 : conj(T[t'][a[b]][f']) * T[t'][c[b]][f']
 *                     mode BASELINE: a[b] < 0 ? 1 : (c[b] ? conj : id)(T[t'][a[b]][f'])
 *   g = fa * fb (complex product, fa first); t' = t when the table has nt snapshots, 0 when it has one; f' likewise over channels.
 *   a_x, c_x: host [nbl] int64 rows of the table (a_x >= -1: -1 gives a row unity gains, as the padding rows of a shard get).
 * sky: host [nt][nbl][nchan] complex128, or NULL: the context's resident slots [t0, t0 + nt) (nbl and nchan the array's).  With
 * sky_c64 != 0 every sky value is rounded to complex64 and back first (a memsave sky promoted to complex128, as numpy does).
 * noise: host [nt][nbl][nchan] complex128 or NULL (zero).  With want_gain != 0, vis = g alone (the gain cube): sky and noise are not read.
 * vis: host [nt][nbl][nchan] complex128.  The cube streams through the device in chunks of whole snapshots (at most 512 MiB per
 * chunk and stream), so device memory stays bounded whatever nt is; stats->kernel_ms sums the chunks' kernels. */
int prisim_gains_apply(prisim_ctx* ctx, int64_t nt, int64_t nbl, int64_t nchan, const prisim_gains_table* ta, int32_t mode_a,
                       const int64_t* a_a, const int64_t* c_a, const prisim_gains_table* tb, int32_t mode_b, const int64_t* a_b,
                       const int64_t* c_b, const double* sky, int64_t t0, int32_t sky_c64, const double* noise, int32_t want_gain,
                       double* vis, prisim_gains_stats* stats);

#ifdef __cplusplus
}
#endif

#endif /* PRISIM_GAINS_H */
