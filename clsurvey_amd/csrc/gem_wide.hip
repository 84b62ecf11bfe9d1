// GEM on sequences of more than 16 tasks: the Gram pass, project2cone2's QP and the projection for up to CLHIP_GEM_WIDE_MAX = 64
// rows (63 memory rows + the current gradient = CLHIP_MAX_TASKS tasks).  Semantics are those of the entries of gem.hip, which
// stay as they are for m <= 16; what differs is where the work lives:
//
//   gram     gem.hip keeps the m rows of a column group and every pair accumulator in registers (136 doubles at m = 16; 64 rows
//            would need 2080).  Here the m rows are cut into 16-row panels and every panel pair (I <= J, 10 at m = 64) is one
//            v_mfma_f64_16x16x4_f64 accumulator tile of 4 doubles per lane.  A wave owns 32 columns per trip: lane l loads 8
//            consecutive floats of row 16 P + (l & 15) from column 8 (l >> 4) on, one row of every panel, i.e. every row is
//            read in whole 128-byte pieces and exactly once; the 8 floats feed 8 k-steps, each of NPAIR MFMAs on operands
//            converted to f64 (a product of two floats is exact in f64; the MFMA accumulates in f64).  Which column sits in
//            which k slot is irrelevant to a Gram matrix as long as both operands use the same map, and A[i][k] / B[k][j] of
//            this MFMA have the same lane map, so ONE register per panel serves as A and as B.  No LDS in the column loop.
//   qp       gem.hip solves on one lane.  Here one workgroup of 256 threads runs the same Goldfarb-Idnani steps with the same
//            decisions (most violated inactive constraint, first on ties; partial / full step; tol 1e-12) and the O(n^2) /
//            O(n^3) pieces spread over its lanes; every decision that a barrier depends on is taken from LDS values that all
//            lanes read after a barrier, so every branch around a barrier is block-uniform.
//   project  the kernels of gem.hip with 63 row indices / coefficients instead of 16.
#include "common.hpp"

namespace {

constexpr int WMAX = CLHIP_GEM_WIDE_MAX;      // rows of a Gram matrix
constexpr int WB = 256;                       // threads per block of every kernel here
constexpr int WAVE_COLS = 32;                 // columns a wave consumes per trip (8 per 16-lane group)
constexpr int BLOCK_COLS = WAVE_COLS * (WB / 64);
constexpr int GRAM_WIDE_BLOCKS = 1024;        // block cap of the Gram pass: one 16 x 16 tile per block and panel pair in ws
constexpr int TILE = 256;                     // doubles of an accumulator tile

struct WideSel { int idx[WMAX]; };
struct WideCoefs { float v[WMAX - 1]; };

typedef double doublex4 __attribute__((ext_vector_type(4)));

__host__ __device__ constexpr int wide_panels(int m) { return (m + 15) / 16; }
__host__ __device__ constexpr int wide_pairs(int m) { return wide_panels(m) * (wide_panels(m) + 1) / 2; }

// 8 consecutive floats of one row of every panel from column c on: two 16-byte loads where the path allows it and the 8 columns
// lie inside n, else guarded scalar loads; rows past m and columns n .. ld-1 are zeros, never loads.
template <int NP>
__device__ __forceinline__ void gram_wide_load(float (&x)[NP][8], const float* const (&rowp)[NP], const bool (&live)[NP], bool vec,
                                               size_t c, size_t n) {
#pragma unroll
    for (int P = 0; P < NP; ++P) {
        if (live[P] && vec && c + 8 <= n) {                 // (16-byte path: G aligned, ld % 4 == 0, c % 8 == 0)
            const float4 a = *reinterpret_cast<const float4*>(rowp[P] + c);
            const float4 b = *reinterpret_cast<const float4*>(rowp[P] + c + 4);
            x[P][0] = a.x; x[P][1] = a.y; x[P][2] = a.z; x[P][3] = a.w;
            x[P][4] = b.x; x[P][5] = b.y; x[P][6] = b.z; x[P][7] = b.w;
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) x[P][e] = (live[P] && c + e < n) ? rowp[P][c + e] : 0.f;
        }
    }
}

// v_mfma_f64_16x16x4_f64: lane l supplies A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]; register g of lane l
// holds D[row = (l >> 4) + 4 g][col = l & 15]  (the f64 form has a C/D map of its own).
//
// partial[block][pair][256]: the block's sum of its four waves' tiles, in the registers' own order (entry 64 g + l).
template <int NP>
__global__ __launch_bounds__(WB) void gram_wide_partial_kernel(const float* __restrict__ G, size_t ld, WideSel sel, int m, size_t n,
                                                               int vec, double* __restrict__ partial) {
    constexpr int NPAIR = NP * (NP + 1) / 2;
    __shared__ double red[WB / 64][TILE];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int r16 = lane & 15, q = lane >> 4;
    const float* rowp[NP];
    bool live[NP];
#pragma unroll
    for (int P = 0; P < NP; ++P) {
        const int r = P * 16 + r16;
        live[P] = r < m;                       // rows m .. 16 NP - 1 are zero operands, never loads
        rowp[P] = G + (size_t)sel.idx[live[P] ? r : 0] * ld;
    }
    doublex4 acc[NPAIR];
#pragma unroll
    for (int k = 0; k < NPAIR; ++k) acc[k] = doublex4{0.0, 0.0, 0.0, 0.0};
    const size_t stride = (size_t)gridDim.x * BLOCK_COLS;
    // the loads of the next trip are issued before this trip's MFMAs (a trip past the end loads nothing and holds zeros)
    size_t c0 = ((size_t)blockIdx.x * (WB / 64) + wave) * WAVE_COLS;
    float x[NP][8], nx[NP][8];
    gram_wide_load<NP>(x, rowp, live, vec != 0, c0 + 8 * (size_t)q, n);
    while (c0 < n) {
        c0 += stride;
        gram_wide_load<NP>(nx, rowp, live, vec != 0, c0 + 8 * (size_t)q, n);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            double d[NP];
#pragma unroll
            for (int P = 0; P < NP; ++P) d[P] = (double)x[P][e];
            int k = 0;
#pragma unroll
            for (int I = 0; I < NP; ++I)
#pragma unroll
                for (int J = I; J < NP; ++J, ++k) acc[k] = __builtin_amdgcn_mfma_f64_16x16x4f64(d[I], d[J], acc[k], 0, 0, 0);
        }
#pragma unroll
        for (int P = 0; P < NP; ++P)
#pragma unroll
            for (int e = 0; e < 8; ++e) x[P][e] = nx[P][e];
    }
    // the four waves' tiles of a pair, added in a fixed order; every wave reaches every barrier (a wave without columns adds zeros)
#pragma unroll
    for (int k = 0; k < NPAIR; ++k) {
#pragma unroll
        for (int g = 0; g < 4; ++g) red[wave][g * 64 + lane] = acc[k][g];
        __syncthreads();
        partial[((size_t)blockIdx.x * NPAIR + k) * TILE + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
        __syncthreads();
    }
}

// Entry E = 256 pair + 64 g + l of the tiles: 16 slices of a block add the per-block partials b = slice, slice + 16, ... of 16
// neighbouring entries (128-byte reads), a fixed tree adds the slices.  Diagonal panels write their upper triangle only and
// mirror it, so the output is bitwise symmetric whatever the matrix core does inside a tile.
__global__ __launch_bounds__(WB) void gram_wide_final_kernel(const double* __restrict__ partial, int nblocks, int m,
                                                             double* __restrict__ out) {
    __shared__ double red[16][16];
    const int NP = wide_panels(m), NPAIR = NP * (NP + 1) / 2;
    const int el = threadIdx.x & 15, slice = threadIdx.x >> 4;
    const int E = blockIdx.x * 16 + el;                                   // < NPAIR * 256 (the grid is NPAIR * 16 blocks)
    const size_t stride = (size_t)NPAIR * TILE;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;                     // four independent chains: four loads in flight per lane
    int b = slice;
    for (; b + 48 < nblocks; b += 64) {
        s0 += partial[(size_t)b * stride + E];
        s1 += partial[(size_t)(b + 16) * stride + E];
        s2 += partial[(size_t)(b + 32) * stride + E];
        s3 += partial[(size_t)(b + 48) * stride + E];
    }
    for (; b < nblocks; b += 16) s0 += partial[(size_t)b * stride + E];
    red[slice][el] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    for (int o = 8; o > 0; o >>= 1) {
        if (slice < o) red[slice][el] += red[slice + o][el];
        __syncthreads();
    }
    if (slice == 0) {
        int I = 0, rem = E / TILE;                                        // pair index -> (I, J), row-major upper triangle
        while (rem >= NP - I) { rem -= NP - I; ++I; }
        const int J = I + rem;
        const int e = E % TILE, g = e >> 6, l = e & 63;
        const int row = I * 16 + (l >> 4) + 4 * g, col = J * 16 + (l & 15);
        if (row < m && col < m && (I != J || row <= col)) {
            out[(size_t)row * m + col] = red[0][el];
            out[(size_t)col * m + row] = red[0][el];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// project2cone2's QP for up to 63 unknowns on one workgroup: the steps of gem_qp_kernel (gem.hip) and oracle/qp_ref.solve_qp.
// Matrices are f64 in LDS with a row stride of 65 doubles: Ginv; A = P, then its Cholesky factor in place, later the
// augmented system [S | rhs] of N*; B = Linv.  ~101 KB of the workgroup's 160 KB.
constexpr int QN = WMAX - 1;
constexpr int QLD = WMAX + 1;

struct QpWide {
    double Ginv[QN * QLD], A[QN * QLD], B[QN * QLD];
    double a[WMAX], x[WMAX], z[WMAX], r[WMAX], u[WMAX + 1];
    int active[WMAX + 1];
    double t;
    int p, drop, full, move;
};

__global__ __launch_bounds__(WB) void gem_qp_wide_kernel(const double* __restrict__ gram, int m, double margin, double eps,
                                                         double* __restrict__ v_out, int* __restrict__ info) {
    __shared__ QpWide W;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = m - 1;                                   // unknowns = memory rows; row / column n = current gradient
    // every wave counts the violated constraints from the same (read-only) Gram row: block-uniform
    const int viol = __popcll(__ballot(lane < n && gram[(size_t)n * m + (lane < n ? lane : 0)] < 0.0));
    if (tid < n) v_out[tid] = 0.0;
    if (tid == 0) { info[0] = viol; info[1] = 0; }
    if (viol == 0) return;
    const double tol = 1e-12;
    double *Ginv = W.Ginv, *A = W.A, *B = W.B, *x = W.x, *z = W.z, *r = W.r, *u = W.u;
    int* active = W.active;
    for (int idx = tid; idx < n * n; idx += WB) {
        const int i = idx / n, j = idx % n;
        A[i * QLD + j] = 0.5 * (gram[(size_t)i * m + j] + gram[(size_t)j * m + i]) + (i == j ? eps : 0.0);
    }
    if (tid < n) W.a[tid] = -gram[(size_t)tid * m + n];    // q = -M g; quadprog minimises 1/2 x^T G x - a^T x with a = q
    if (tid <= WMAX) active[tid] = 0;
    __syncthreads();
    // Cholesky A = L L^T in place (lower triangle), column by column: lane i of column j forms the dot products of
    // qp_inverse_spd in the same order; the column's entries are written after everybody has read its diagonal
    for (int j = 0; j < n; ++j) {
        const int i = j + tid;
        double val = 0.0;
        if (i < n) {
            double s = A[i * QLD + j], d = A[j * QLD + j];
            for (int k = 0; k < j; ++k) {
                s -= A[i * QLD + k] * A[j * QLD + k];
                d -= A[j * QLD + k] * A[j * QLD + k];
            }
            val = (i == j) ? sqrt(d) : s / sqrt(d);
        }
        __syncthreads();
        if (i < n) A[i * QLD + j] = val;
        __syncthreads();
    }
    // Linv by forward substitution, one column per lane
    if (tid < n) {
        const int c = tid;
        for (int i = 0; i < n; ++i) {
            if (i < c) { B[i * QLD + c] = 0.0; continue; }
            double s = (i == c) ? 1.0 : 0.0;
            for (int k = c; k < i; ++k) s -= A[i * QLD + k] * B[k * QLD + c];
            B[i * QLD + c] = s / A[i * QLD + i];
        }
    }
    __syncthreads();
    for (int idx = tid; idx < n * n; idx += WB) {          // Ginv = Linv^T Linv
        const int i = idx / n, j = idx % n;
        double s = 0.0;
        for (int k = (i > j ? i : j); k < n; ++k) s += B[k * QLD + i] * B[k * QLD + j];
        Ginv[i * QLD + j] = s;
    }
    __syncthreads();
    if (tid < n) {
        double s = 0.0;
        for (int j = 0; j < n; ++j) s += Ginv[tid * QLD + j] * W.a[j];
        x[tid] = s;                                        // unconstrained minimum
    }
    __syncthreads();
    int na = 0;
    for (int it = 0; it < 200; ++it) {
        // constraints are v_i >= margin: slack s_i = x_i - margin; most violated inactive one, the first of equals
        if (wave == 0) {
            bool act = false;
            for (int k = 0; k < na; ++k) act |= active[k] == lane;
            const double si = lane < n ? x[lane] - margin : 0.0;
            const bool cand = lane < n && !act && si < -tol * fmax(1.0, fabs(margin));
            double best = cand ? si : INFINITY;
            int bi = cand ? lane : 64;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double ob = __shfl_xor(best, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                if (ob < best || (ob == best && oi < bi)) { best = ob; bi = oi; }
            }
            if (lane == 0) { W.p = bi < 64 ? bi : -1; u[na] = 0.0; }
        }
        __syncthreads();
        const int p = W.p;                                 // block-uniform from here on
        if (p < 0) {
            if (tid < n) v_out[tid] = x[tid];
            return;
        }
        for (int inner = 0; inner < 200; ++inner) {
            if (na > 0) {
                // r = N* e_p = S^-1 Ginv[active][p] with S = Ginv[active][active]: Gaussian elimination with partial pivoting
                // on [S | rhs] (column na), as qp_solve does for the one right-hand side that is used
                for (int idx = tid; idx < na * (na + 1); idx += WB) {
                    const int i = idx / (na + 1), j = idx % (na + 1);
                    A[i * QLD + j] = Ginv[active[i] * QLD + (j < na ? active[j] : p)];
                }
                __syncthreads();
                for (int c = 0; c < na; ++c) {
                    // pivot: the first largest |S[r][c]|, r >= c; every wave finds it from the same LDS values
                    const int rr = c + lane;
                    double best = rr < na ? fabs(A[rr * QLD + c]) : -1.0;
                    int piv = rr < na ? rr : 1 << 20;
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) {
                        const double ob = __shfl_xor(best, o, 64);
                        const int oi = __shfl_xor(piv, o, 64);
                        if (ob > best || (ob == best && oi < piv)) { best = ob; piv = oi; }
                    }
                    __syncthreads();                       // every wave has read column c before rows move
                    if (piv != c && tid >= c && tid <= na) {
                        const double tmp = A[c * QLD + tid];
                        A[c * QLD + tid] = A[piv * QLD + tid];
                        A[piv * QLD + tid] = tmp;
                    }
                    __syncthreads();
                    // rows c + 1 .. na - 1, columns c + 1 .. na (column c itself is never read again and stays as it is)
                    const int k = c + 1 + lane;
                    const double pivot = A[c * QLD + c];
                    for (int row = c + 1 + wave; row < na; row += WB / 64) {
                        const double f = A[row * QLD + c] / pivot;
                        if (k <= na) A[row * QLD + k] -= f * A[c * QLD + k];
                    }
                    __syncthreads();
                }
                if (wave == 0) {
                    // back substitution, column by column: lane i keeps the right-hand side of row i
                    double bi = lane < na ? A[lane * QLD + na] : 0.0;
                    for (int row = na - 1; row >= 0; --row) {
                        const double xr = __shfl(bi, row, 64) / A[row * QLD + row];
                        if (lane == row) bi = xr;
                        else if (lane < row) bi -= A[lane * QLD + row] * xr;
                    }
                    if (lane < na) r[lane] = bi;
                }
                __syncthreads();
                if (tid < n) {                             // z = H e_p = Ginv[:, p] - Ginv[:, active] r
                    double s = Ginv[tid * QLD + p];
                    for (int k = 0; k < na; ++k) s -= Ginv[tid * QLD + active[k]] * r[k];
                    z[tid] = s;
                }
            } else if (tid < n) {
                z[tid] = Ginv[tid * QLD + p];
            }
            __syncthreads();
            if (wave == 0) {
                // step lengths: t1 = the first smallest u_j / r_j over r_j > tol (the constraint to drop), t2 to the constraint
                const bool ok = lane < na && r[lane] > tol;
                double best = ok ? u[lane] / r[lane] : INFINITY;
                int drop = ok ? lane : 64;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const double ob = __shfl_xor(best, o, 64);
                    const int oi = __shfl_xor(drop, o, 64);
                    if (ob < best || (ob == best && oi < drop)) { best = ob; drop = oi; }
                }
                if (lane == 0) {
                    const double t1 = best;                // (INFINITY when nothing can be dropped)
                    double t2 = INFINITY;
                    const double zn = z[p], sp = x[p] - margin;
                    if (zn > tol) t2 = -sp / zn;
                    const double t = fmin(t1, t2);
                    W.t = t;
                    W.drop = t1 < INFINITY ? drop : -1;
                    W.full = t == t2;
                    W.move = t2 < INFINITY;
                }
            }
            __syncthreads();
            const double t = W.t;
            const int drop = W.drop, full = W.full, move = W.move;
            if (!(t < INFINITY)) {                          // infeasible
                if (tid == 0) info[1] = 2;
                return;
            }
            if (move && tid < n) x[tid] += t * z[tid];
            if (tid < na) u[tid] -= t * r[tid];
            else if (tid == na) u[na] += t;
            __syncthreads();
            if (full) {                                     // full step: p joins the active set
                if (tid == 0) active[na] = p;
                ++na;
                __syncthreads();
                break;
            }
            // partial step: the constraint at position drop leaves, p is tried again
            int a_next = 0;
            double u_next = 0.0;
            const bool mine = tid >= drop && tid < na;
            if (mine) { a_next = active[tid + 1]; u_next = u[tid + 1]; }
            __syncthreads();
            if (mine) { active[tid] = a_next; u[tid] = u_next; }
            --na;
            __syncthreads();
            if (inner == 199) {
                if (tid == 0) info[1] = 1;
                return;
            }
        }
    }
    if (tid == 0) info[1] = 1;
}

// ---------------------------------------------------------------------------------------------------------
// project_kernel / project_dev_kernel of gem.hip for up to 63 rows: s = f64(g[c]); s += f64(v_i) f64(G_i[c]) in row order, one
// rounding to fp32.
template <bool VEC>
__global__ __launch_bounds__(WB) void project_wide_kernel(const float* __restrict__ G, size_t ld, WideSel sel, WideCoefs cf, int m,
                                                          const float* __restrict__ g, float* __restrict__ out, size_t n) {
    const size_t stride = (size_t)gridDim.x * WB;
    const size_t n4 = VEC ? n / 4 : 0;
    for (size_t c4 = (size_t)blockIdx.x * WB + threadIdx.x; c4 < n4; c4 += stride) {
        const float4 gv = reinterpret_cast<const float4*>(g)[c4];
        double s0 = (double)gv.x, s1 = (double)gv.y, s2 = (double)gv.z, s3 = (double)gv.w;
        for (int i = 0; i < m; ++i) {
            const float4 r = reinterpret_cast<const float4*>(G + (size_t)sel.idx[i] * ld)[c4];
            const double vi = (double)cf.v[i];
            s0 += vi * (double)r.x; s1 += vi * (double)r.y; s2 += vi * (double)r.z; s3 += vi * (double)r.w;
        }
        reinterpret_cast<float4*>(out)[c4] = make_float4((float)s0, (float)s1, (float)s2, (float)s3);
    }
    for (size_t c = n4 * 4 + (size_t)blockIdx.x * WB + threadIdx.x; c < n; c += stride) {
        double s = (double)g[c];
        for (int i = 0; i < m; ++i) s += (double)cf.v[i] * (double)G[(size_t)sel.idx[i] * ld + c];
        out[c] = (float)s;
    }
}

template <bool VEC>
__global__ __launch_bounds__(WB) void project_dev_wide_kernel(const float* __restrict__ G, size_t ld, WideSel sel,
                                                              const double* __restrict__ v, const int* __restrict__ info, int m,
                                                              const float* __restrict__ g, float* __restrict__ out, size_t n) {
    if (info[0] == 0 && out == g) return;                   // no violated constraint: the gradient stays as it is (block-uniform)
    const int rows = info[0] == 0 ? 0 : m;                  // ... and out != g: out = g bit for bit, no memory row is read
    __shared__ double cv[WMAX];
    if ((int)threadIdx.x < rows) cv[threadIdx.x] = (double)(float)v[threadIdx.x];   // v rounded to fp32 as torch.Tensor(x) does downstream
    __syncthreads();
    const size_t stride = (size_t)gridDim.x * WB;
    const size_t n4 = VEC ? n / 4 : 0;
    for (size_t c4 = (size_t)blockIdx.x * WB + threadIdx.x; c4 < n4; c4 += stride) {
        const float4 gv = reinterpret_cast<const float4*>(g)[c4];
        double s0 = (double)gv.x, s1 = (double)gv.y, s2 = (double)gv.z, s3 = (double)gv.w;
        for (int i = 0; i < rows; ++i) {
            const float4 r = reinterpret_cast<const float4*>(G + (size_t)sel.idx[i] * ld)[c4];
            s0 += cv[i] * (double)r.x; s1 += cv[i] * (double)r.y; s2 += cv[i] * (double)r.z; s3 += cv[i] * (double)r.w;
        }
        reinterpret_cast<float4*>(out)[c4] = make_float4((float)s0, (float)s1, (float)s2, (float)s3);
    }
    for (size_t c = n4 * 4 + (size_t)blockIdx.x * WB + threadIdx.x; c < n; c += stride) {
        double s = (double)g[c];
        for (int i = 0; i < rows; ++i) s += cv[i] * (double)G[(size_t)sel.idx[i] * ld + c];
        out[c] = (float)s;
    }
}

int gram_wide_blocks(size_t n) {
    const size_t b = (n + BLOCK_COLS - 1) / BLOCK_COLS;
    return b > (size_t)GRAM_WIDE_BLOCKS ? GRAM_WIDE_BLOCKS : (int)b;
}

}  // namespace

extern "C" {

size_t clhip_gem_gram_wide_ws(int m) {
    if (m < 1 || m > WMAX) return 0;
    return (size_t)GRAM_WIDE_BLOCKS * wide_pairs(m) * TILE * sizeof(double);
}

// out_f64[m*m] (device) = Gram matrix of rows row_idx[0..m) of G (each row n floats, stride ld floats), 1 <= m <= 64
int clhip_gem_gram_wide(const float* G, size_t ld, const int* row_idx_host, int m, size_t n, double* out_f64, void* ws,
                        size_t ws_bytes, void* stream) {
    if (!G || !row_idx_host || !out_f64 || !ws || m < 1 || m > WMAX || n == 0 || ws_bytes < clhip_gem_gram_wide_ws(m))
        return CLHIP_EINVAL;
    WideSel sel{};
    for (int i = 0; i < m; ++i) sel.idx[i] = row_idx_host[i];
    hipStream_t s = as_stream(stream);
    const int vec = aligned16(G) && (ld % 4 == 0);
    const int blocks = gram_wide_blocks(n);                 // a function of n alone: the result does not depend on the run
    double* partial = static_cast<double*>(ws);
    switch (wide_panels(m)) {
#define CASE(NP_) case NP_: hipLaunchKernelGGL((gram_wide_partial_kernel<NP_>), dim3(blocks), dim3(WB), 0, s, G, ld, sel, m, n, vec, partial); break;
        CASE(1) CASE(2) CASE(3) CASE(4)
#undef CASE
    }
    CLHIP_LAUNCH_CHECK();
    hipLaunchKernelGGL(gram_wide_final_kernel, dim3(wide_pairs(m) * 16), dim3(WB), 0, s, partial, blocks, m, out_f64);
    CLHIP_LAUNCH_CHECK();
    return 0;
}

size_t clhip_gem_qp_wide_ws(int m) {
    (void)m;
    return 0;                                               // the solver's matrices live in LDS
}

int clhip_gem_qp_wide(const double* gram_f64, int m, double margin, double eps, double* v_out_f64, int* info_i32, void* ws,
                      size_t ws_bytes, void* stream) {
    (void)ws;
    if (!gram_f64 || !v_out_f64 || !info_i32 || m < 2 || m > WMAX || ws_bytes < clhip_gem_qp_wide_ws(m)) return CLHIP_EINVAL;
    hipLaunchKernelGGL(gem_qp_wide_kernel, dim3(1), dim3(WB), 0, as_stream(stream), gram_f64, m, margin, eps, v_out_f64, info_i32);
    CLHIP_LAUNCH_CHECK();
    return 0;
}

int clhip_gem_project_wide(const float* G, size_t ld, const int* row_idx_host, const float* v_host, int m, const float* g,
                           float* out, size_t n, void* stream) {
    if (!G || !row_idx_host || !v_host || !g || !out || m < 1 || m > WMAX - 1 || n == 0) return CLHIP_EINVAL;
    WideSel sel{}; WideCoefs cf{};
    for (int i = 0; i < m; ++i) { sel.idx[i] = row_idx_host[i]; cf.v[i] = v_host[i]; }
    if (aligned16(G) && (ld % 4 == 0) && aligned16(g) && aligned16(out))
        hipLaunchKernelGGL(project_wide_kernel<true>, dim3(ew_grid(n / 4 + 1, WB)), dim3(WB), 0, as_stream(stream), G, ld, sel, cf, m, g, out, n);
    else
        hipLaunchKernelGGL(project_wide_kernel<false>, dim3(ew_grid(n, WB)), dim3(WB), 0, as_stream(stream), G, ld, sel, cf, m, g, out, n);
    CLHIP_LAUNCH_CHECK();
    return 0;
}

int clhip_gem_project_dev_wide(const float* G, size_t ld, const int* row_idx_host, const double* v_dev_f64, const int* info_dev,
                               int m, const float* g, float* out, size_t n, void* stream) {
    if (!G || !row_idx_host || !v_dev_f64 || !info_dev || !g || !out || m < 1 || m > WMAX - 1 || n == 0) return CLHIP_EINVAL;
    WideSel sel{};
    for (int i = 0; i < m; ++i) sel.idx[i] = row_idx_host[i];
    if (aligned16(G) && (ld % 4 == 0) && aligned16(g) && aligned16(out))
        hipLaunchKernelGGL(project_dev_wide_kernel<true>, dim3(ew_grid(n / 4 + 1, WB)), dim3(WB), 0, as_stream(stream), G, ld, sel,
                           v_dev_f64, info_dev, m, g, out, n);
    else
        hipLaunchKernelGGL(project_dev_wide_kernel<false>, dim3(ew_grid(n, WB)), dim3(WB), 0, as_stream(stream), G, ld, sel,
                           v_dev_f64, info_dev, m, g, out, n);
    CLHIP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
