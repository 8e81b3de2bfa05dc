// gs_ensemble.h -- ensembles: `members` independent grids of one shape, each with its own parameters, advanced in shared
// launches (gs_ensemble_run, gs_ensemble.cpp).  Two forms, both made of the per-cell code of gs_lds_resident.h:
//   gs_ens_resident_k  one workgroup per member for the whole call: the member is loaded into LDS once, advanced `steps`
//                      times LDS -> LDS with one barrier per step, and stored once (gs_run_resident_k with a member
//                      coordinate, up to 8 cells per thread and 160 KiB of LDS: gs_ens_resident_cpt);
//   gs_ens_tile_k      K <= 8 steps per launch on LDS-resident windows (gs_run_tile_k with a member coordinate): grid =
//                      members x windows per member; a window never reads across its member's edge -- cells outside
//                      the member are zeros, exactly as cells outside the grid are for a lone Species.
// Under the periodic rule (zero_halo = 2) the resident form keeps its ring filled with the opposite edge (ring_put) and
// the windowed form is gs_ens_tile_pk, whose windows read their member's cells at wrapped coordinates.  Under the zero-flux
// rule (zero_halo = 3) the resident form keeps its ring filled with the edge cells' own values (ring_put_edge) and the
// windowed form is gs_ens_tile_nk (tile_steps<ZH = 3>).
// A workgroup belongs to ONE member, so its parameters are wave-uniform: they are read from the device table with scalar
// loads (constant address space) into SGPRs.  Member offsets are 64-bit.
// Listed forms (gs_ens_resident_lk / _lpk / _lnk, gs_ens_tile_lk / _lpk / _lnk): the same bodies for an ensemble with an
// active set (gs_members_set_active).  The grid covers the ACTIVE members only, and a workgroup takes its member from a
// device list of their indices (u32, ascending; the kernels' second argument) with one scalar load, where its twin
// computes it from the workgroup index: the member stays wave-uniform.  GsEnsArgs::first is then a position in the list.
// Noise forms (gs_ens_resident_zk / _zpk / _znk, gs_ens_tile_zk / _zpk / _znk; gs_members_set_noise): the same bodies with
// react_noise (gs_cell.h) on the outputs of every cell a step computes inside the member -- the apron cells of a window at
// every level included -- before the value is published to LDS or stored.  A cell draws at its member-local (row, column),
// under the periodic rule at the wrapped one, with the key of the member's own step: the member's seed, sigmas and step
// offset come from a second device table (GsEnsNoise, one s_load_dwordx8), the key is formed on the device once per step
// from wave-uniform words (noise_key_uniform).  The second argument, GsEnsNoiseArgs, carries a nullable list of active
// members: one form serves ensembles with and without an active set.  Built in the noise translation units (gs_step_noise.hip)
// only: the other objects hold none of them.
// Part of the gfx950 step kernels: included by gs_step_kernels.hip (the plain and listed forms) and gs_step_noise.hip (the
// noise forms) behind gs_step_flavour.h (GS_MATH_FUSED, GS_SUFFIX, GS_TAP) and gs_lds_resident.h, once per arithmetic
// flavour; the launchers' shared bodies are in gs_ens_launch.h.  Not a header to include elsewhere.
#pragma once

namespace {

typedef __attribute__((address_space(4))) const GsEnsParams GsEnsParamsConst;

// The GsStepArgs the per-cell code reads, for member `member` (rows, columns, boundary rule, parameters, planes).
__device__ __forceinline__ GsStepArgs ens_member_args(const GsEnsArgs &e, int64_t member)
{
    GsStepArgs a{};
    GsEnsParamsConst *q = (GsEnsParamsConst *)e.params + member; // s_load: member is wave-uniform
    const int64_t off = member * ((int64_t)e.rows * e.cols);
    a.in_u = e.in_u + off;
    a.in_v = e.in_v + off;
    a.out_u = e.out_u + off;
    a.out_v = e.out_v + off;
    a.rows = e.rows;
    a.cols = e.cols;
    a.pitch = e.cols;
    a.zero_halo = e.zero_halo;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) a.w[i][j] = q->w[i][j];
    a.du = q->du;
    a.dv = q->dv;
    a.feed = q->feed;
    a.feed_plus_kill = q->feed_plus_kill;
    a.dt = q->dt;
    return a;
}

typedef __attribute__((address_space(4))) const GsEnsNoise GsEnsNoiseConst;
// The noise of member `member` at the first step of a launch (scalar loads: member is wave-uniform).
__device__ __forceinline__ MemberNoise ens_member_noise(const GsEnsNoiseArgs &z, int64_t member)
{
    GsEnsNoiseConst *q = (GsEnsNoiseConst *)z.table + member;
    MemberNoise mn;
    mn.sigma_u = q->sigma_u;
    mn.sigma_v = q->sigma_v;
    mn.seed_lo = q->seed_lo;
    mn.seed_hi = q->seed_hi;
    mn.step = z.step0 + ((uint64_t)q->offset_hi << 32 | q->offset_lo);
    return mn;
}

// Resident form.  The LDS layout and the step loop are gs_run_resident_k's: 4 planes of (rows + 2) x (cols + 2) floats
// with a ring of zeros, thread t owning cells t, t + blockDim.x, ... (CPT of them at most).  The host sizes the
// workgroup to the waves the member's cells need (an 8 x 16 member: 2 waves), so small members share a CU.
// (The body is a macro so that the kernel of the clipped and zero-halo rules keeps its code: as a function called from two
// kernels it compiled one instruction apart.)  MEMBER: the workgroup's member, GS_ENS_MEMBER_OF_GROUP or GS_ENS_MEMBER_LISTED,
// or GS_ENS_MEMBER_NOISE in the noise forms (NZ = 1), whose hooks GS_ENS_NZ_*_1 stand where the others' expand to nothing.
typedef __attribute__((address_space(4))) const uint32_t GsEnsListConst;
// The member of workgroup (or window group) G of a launch: counted from GsEnsArgs::first, or entry first + G of the list of
// active members (one s_load_dword: G is wave-uniform).
#define GS_ENS_MEMBER_OF_GROUP(G) (e.first + (int64_t)(G))
#define GS_ENS_MEMBER_LISTED(G) ((int64_t)((GsEnsListConst *)list)[e.first + (int64_t)(G)])
#define GS_ENS_MEMBER_NOISE(G) (z.list ? (int64_t)((GsEnsListConst *)z.list)[e.first + (int64_t)(G)] : e.first + (int64_t)(G))
// the member's noise, once per workgroup
#define GS_ENS_NZ_MEMBER_0(M)
#define GS_ENS_NZ_MEMBER_1(M) const MemberNoise mn = ens_member_noise(z, M);
// the key of step s, once per step
#define GS_ENS_NZ_STEP_0
#define GS_ENS_NZ_STEP_1 const uint32_t zkey = member_key(mn, s);
// a cell's draw at its member coordinates (rc[k], unpacked inside the step loop: see the ring's remark below)
#define GS_ENS_NZ_CELL_0(k)
#define GS_ENS_NZ_CELL_1(k)                                                                                                  \
    {                                                                                                                        \
        int x = rc[k];                                                                                                       \
        asm volatile("" : "+v"(x));                                                                                          \
        const uint32_t zr[1] = {(uint32_t)(x >> 16)};                                                                        \
        float zu[1] = {nu}, zv[1] = {nv};                                                                                    \
        member_noise<1>(mn, zkey, zr, (uint32_t)(x & 0xffff), zu, zv);                                                          \
        nu = zu[0];                                                                                                          \
        nv = zv[0];                                                                                                          \
    }
#define GS_ENS_RESIDENT_BODY(CPT, FAST, ZH, MEMBER, NZ)                                                                        \
    if ((FAST & 1) && !GS_MATH_FUSED) __builtin_amdgcn_s_setreg(1 | (9 << 6), 0); /* half_diff: MODE.IEEE = 0 */             \
    extern __shared__ float lds[];                                                                                           \
    const GsStepArgs a = ens_member_args(e, MEMBER);                                                                         \
    GS_ENS_NZ_MEMBER_##NZ(MEMBER)                                                                                            \
    const int cells = a.rows * a.cols, cols = a.cols, P = cols + 2, plane = (a.rows + 2) * P;                                \
    const int nthreads = (int)blockDim.x;                                                                                    \
    for (int i = threadIdx.x; i < 4 * plane; i += nthreads) lds[i] = 0.0f; /* the rings (and everything else) */             \
    __syncthreads();                                                                                                         \
    int o[CPT], rc[CPT]; /* rc (ZH = 2, 3: the ring of the periodic / zero-flux rule): row << 16 | column */               \
    bool live[CPT];                                                                                                          \
    float E[CPT][8];                                                                                                         \
_Pragma("unroll")                                                                                                            \
    for (int k = 0; k < CPT; ++k) {                                                                                          \
        const int idx = (int)threadIdx.x + k * nthreads;                                                                     \
        live[k] = idx < cells;                                                                                               \
        const int r = live[k] ? idx / cols : 0, c = live[k] ? idx - r * cols : 0;                                            \
        o[k] = (r + 1) * P + c + 1;                                                                                          \
        if (ZH == 0) border_weights(a, r, c, E[k]);                                                                          \
        if constexpr (ZH >= 2 || NZ) rc[k] = r << 16 | c;                                                                    \
        if (live[k]) {                                                                                                       \
            lds[o[k]] = a.in_u[idx];                                                                                         \
            lds[2 * plane + o[k]] = a.in_v[idx];                                                                             \
            if (ZH >= 2 && on_border(a.rows, cols, r, c)) {                                                                  \
                if constexpr (ZH == 3) {                                                                                     \
                    ring_put_edge(lds, P, a.rows, cols, r, c, lds[o[k]]);                                                    \
                    ring_put_edge(lds + 2 * plane, P, a.rows, cols, r, c, lds[2 * plane + o[k]]);                            \
                } else {                                                                                                     \
                    ring_put(lds, P, a.rows, cols, r, c, lds[o[k]]);                                                         \
                    ring_put(lds + 2 * plane, P, a.rows, cols, r, c, lds[2 * plane + o[k]]);                                 \
                }                                                                                                            \
            }                                                                                                                \
        }                                                                                                                    \
    }                                                                                                                        \
    __syncthreads();                                                                                                         \
    int cur = 0;                                                                                                             \
    for (int s = 0; s < steps; ++s) {                                                                                        \
        const float *su = lds + cur * plane, *sv = lds + (2 + cur) * plane;                                                  \
        float *du = lds + (cur ^ 1) * plane, *dv = lds + (2 + (cur ^ 1)) * plane;                                            \
        GS_ENS_NZ_STEP_##NZ                                                                                                  \
_Pragma("unroll")                                                                                                            \
        for (int k = 0; k < CPT; ++k) {                                                                                      \
            if (!live[k]) continue;                                                                                          \
            Row3 R[3];                                                                                                       \
_Pragma("unroll")                                                                                                            \
            for (int i = 0; i < 3; ++i) {                                                                                    \
                const int q = o[k] + (i - 1) * P;                                                                            \
                R[i].u[0] = su[q - 1]; R[i].u[1] = su[q]; R[i].u[2] = su[q + 1];                                             \
                R[i].v[0] = sv[q - 1]; R[i].v[1] = sv[q]; R[i].v[2] = sv[q + 1];                                             \
            }                                                                                                                \
            float nu, nv;                                                                                                    \
            if (ZH == 0)                                                                                                     \
                cell_border<FAST>(a, E[k], R[0], R[1], R[2], nu, nv);                                                        \
            else                                                                                                             \
                cell<false, FAST, Row3>(a, R[0], R[1], R[2], 1, true, true, 0u, 0u, nu, nv);                                 \
            GS_ENS_NZ_CELL_##NZ(k)                                                                                           \
            du[o[k]] = nu;                                                                                                   \
            dv[o[k]] = nv;                                                                                                   \
            if constexpr (ZH >= 2) {                                                                                         \
                /* (opaque: the border tests of all CPT cells, hoisted out of the step loop, would hold SGPR lane masks) */  \
                int x = rc[k];                                                                                               \
                asm volatile("" : "+v"(x));                                                                                  \
                const int r = x >> 16, c = x & 0xffff;                                                                       \
                if (on_border(a.rows, cols, r, c)) {                                                                         \
                    if constexpr (ZH == 3) {                                                                                 \
                        ring_put_edge(du, P, a.rows, cols, r, c, nu);                                                        \
                        ring_put_edge(dv, P, a.rows, cols, r, c, nv);                                                        \
                    } else {                                                                                                 \
                        ring_put(du, P, a.rows, cols, r, c, nu);                                                             \
                        ring_put(dv, P, a.rows, cols, r, c, nv);                                                             \
                    }                                                                                                        \
                }                                                                                                            \
            }                                                                                                                \
        }                                                                                                                    \
        __syncthreads();                                                                                                     \
        cur ^= 1;                                                                                                            \
    }                                                                                                                        \
    float *gu = to_out ? a.out_u : const_cast<float *>(a.in_u);                                                              \
    float *gv = to_out ? a.out_v : const_cast<float *>(a.in_v);                                                              \
_Pragma("unroll")                                                                                                            \
    for (int k = 0; k < CPT; ++k)                                                                                            \
        if (live[k]) {                                                                                                       \
            const int idx = (int)threadIdx.x + k * nthreads;                                                                 \
            gu[idx] = lds[cur * plane + o[k]];                                                                               \
            gv[idx] = lds[(2 + cur) * plane + o[k]];                                                                         \
        }

template <int CPT, int FAST, int ZH>
__global__ __launch_bounds__(1024) void GS_SUFFIX(gs_ens_resident_k)(GsEnsArgs e, int steps, int to_out)
{
    GS_ENS_RESIDENT_BODY(CPT, FAST, ZH, GS_ENS_MEMBER_OF_GROUP(blockIdx.x), 0)
}
// The periodic rule's instances (GsEnsArgs::zero_halo = 2), kernels of their own name.
template <int CPT, int FAST>
__global__ __launch_bounds__(1024) void GS_SUFFIX(gs_ens_resident_pk)(GsEnsArgs e, int steps, int to_out)
{
    GS_ENS_RESIDENT_BODY(CPT, FAST, 2, GS_ENS_MEMBER_OF_GROUP(blockIdx.x), 0)
}
// The zero-flux rule's instances (GsEnsArgs::zero_halo = 3), kernels of their own name.
template <int CPT, int FAST>
__global__ __launch_bounds__(1024) void GS_SUFFIX(gs_ens_resident_nk)(GsEnsArgs e, int steps, int to_out)
{
    GS_ENS_RESIDENT_BODY(CPT, FAST, 3, GS_ENS_MEMBER_OF_GROUP(blockIdx.x), 0)
}
// The listed forms: the member from the list of active members (the second argument).
template <int CPT, int FAST, int ZH>
__global__ __launch_bounds__(1024) void GS_SUFFIX(gs_ens_resident_lk)(GsEnsArgs e, const uint32_t *list, int steps, int to_out)
{
    GS_ENS_RESIDENT_BODY(CPT, FAST, ZH, GS_ENS_MEMBER_LISTED(blockIdx.x), 0)
}
template <int CPT, int FAST>
__global__ __launch_bounds__(1024) void GS_SUFFIX(gs_ens_resident_lpk)(GsEnsArgs e, const uint32_t *list, int steps, int to_out)
{
    GS_ENS_RESIDENT_BODY(CPT, FAST, 2, GS_ENS_MEMBER_LISTED(blockIdx.x), 0)
}
template <int CPT, int FAST>
__global__ __launch_bounds__(1024) void GS_SUFFIX(gs_ens_resident_lnk)(GsEnsArgs e, const uint32_t *list, int steps, int to_out)
{
    GS_ENS_RESIDENT_BODY(CPT, FAST, 3, GS_ENS_MEMBER_LISTED(blockIdx.x), 0)
}
// The noise forms: the member's noise from the table of the second argument, the member from its nullable list.
template <int CPT, int FAST, int ZH>
__global__ __launch_bounds__(1024) void GS_SUFFIX(gs_ens_resident_zk)(GsEnsArgs e, GsEnsNoiseArgs z, int steps, int to_out)
{
    GS_ENS_RESIDENT_BODY(CPT, FAST, ZH, GS_ENS_MEMBER_NOISE(blockIdx.x), 1)
}
template <int CPT, int FAST>
__global__ __launch_bounds__(1024) void GS_SUFFIX(gs_ens_resident_zpk)(GsEnsArgs e, GsEnsNoiseArgs z, int steps, int to_out)
{
    GS_ENS_RESIDENT_BODY(CPT, FAST, 2, GS_ENS_MEMBER_NOISE(blockIdx.x), 1)
}
template <int CPT, int FAST>
__global__ __launch_bounds__(1024) void GS_SUFFIX(gs_ens_resident_znk)(GsEnsArgs e, GsEnsNoiseArgs z, int steps, int to_out)
{
    GS_ENS_RESIDENT_BODY(CPT, FAST, 3, GS_ENS_MEMBER_NOISE(blockIdx.x), 1)
}
#undef GS_ENS_RESIDENT_BODY
#undef GS_ENS_NZ_MEMBER_0
#undef GS_ENS_NZ_MEMBER_1
#undef GS_ENS_NZ_STEP_0
#undef GS_ENS_NZ_STEP_1
#undef GS_ENS_NZ_CELL_0
#undef GS_ENS_NZ_CELL_1

// Windowed form: gs_run_tile_k's load, K steps (tile_steps) and store, for window `blockIdx.x % windows` of member
// `first + blockIdx.x / windows`.
// (The body is a macro, like the resident form's, so that gs_ens_tile_k keeps its code beside its listed twin.)
// (NZ = 1, the noise form: the member's noise, and tile_steps' NOISE = 1 with it as its last argument)
#define GS_ENS_TILE_NZ_MEMBER_0(M)
#define GS_ENS_TILE_NZ_MEMBER_1(M) const MemberNoise mn = ens_member_noise(z, M);
#define GS_ENS_TILE_NZ_T_0
#define GS_ENS_TILE_NZ_T_1 , 1
#define GS_ENS_TILE_NZ_A_0
#define GS_ENS_TILE_NZ_A_1 , mn
#define GS_ENS_TILE_BODY(RPW, FAST, MEMBER, NZ)                                                                               \
    if ((FAST & 1) && !GS_MATH_FUSED) __builtin_amdgcn_s_setreg(1 | (9 << 6), 0); /* half_diff: MODE.IEEE = 0 */             \
    extern __shared__ float lds[];                                                                                           \
    const int m = (int)(blockIdx.x / (unsigned)windows), win = (int)blockIdx.x - m * windows;                                \
    const GsStepArgs a = ens_member_args(e, MEMBER(m));                                                                      \
    GS_ENS_TILE_NZ_MEMBER_##NZ(MEMBER(m))                                                                                    \
    constexpr int H = tile_rows(RPW);                                                                                        \
    const int lane = threadIdx.x & 63;                                                                                       \
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);                                                       \
    const int HO = H - 2 * K, WO = kTileCols - 2 * K; /* output rows / columns per window */                                 \
    const int tiles_c = (a.cols + WO - 1) / WO;                                                                              \
    const int tr = win / tiles_c, tc = win - tr * tiles_c;                                                                   \
    const int gr0 = tr * HO - K, gc0 = tc * WO - K; /* member coordinates of window cell (0, 0) */                           \
    const int gr = gr0 + wave * RPW, gc = gc0 + lane; /* this lane's first cell */                                           \
    /* load; cells outside the member are zeros (and stay zeros: tile_steps) */                                              \
    float u[RPW], v[RPW];                                                                                                    \
    const int cc = min(max(gc, 0), a.cols - 1);                                                                              \
_Pragma("unroll")                                                                                                            \
    for (int i = 0; i < RPW; ++i) {                                                                                          \
        const ptrdiff_t g = (ptrdiff_t)min(max(gr + i, 0), a.rows - 1) * a.pitch + cc;                                       \
        const bool in = gr + i >= 0 && gr + i < a.rows && gc >= 0 && gc < a.cols;                                            \
        u[i] = in ? a.in_u[g] : 0.0f;                                                                                        \
        v[i] = in ? a.in_v[g] : 0.0f;                                                                                        \
    }                                                                                                                        \
    const bool edge = gr0 <= 0 || gc0 <= 0 || gr0 + H >= a.rows || gc0 + kTileCols >= a.cols;                                \
    /* (a.zero_halo is 0 or 1 here: the periodic rule runs gs_ens_tile_pk) */                                                \
    if (!edge)                                                                                                               \
        tile_steps<RPW, false, FAST, -1 GS_ENS_TILE_NZ_T_##NZ>(a, lds, K, gr, gc, wave, lane, u, v GS_ENS_TILE_NZ_A_##NZ);   \
    else if (a.zero_halo)                                                                                                    \
        tile_steps<RPW, true, FAST, 1 GS_ENS_TILE_NZ_T_##NZ>(a, lds, K, gr, gc, wave, lane, u, v GS_ENS_TILE_NZ_A_##NZ);     \
    else                                                                                                                     \
        tile_steps<RPW, true, FAST, 0 GS_ENS_TILE_NZ_T_##NZ>(a, lds, K, gr, gc, wave, lane, u, v GS_ENS_TILE_NZ_A_##NZ);     \
    /* store the window shrunk by K, where it lies in the member */                                                          \
    if (lane >= K && lane < kTileCols - K && gc < a.cols) {                                                                  \
_Pragma("unroll")                                                                                                            \
        for (int i = 0; i < RPW; ++i) {                                                                                      \
            const int wr = wave * RPW + i;                                                                                   \
            if (wr >= K && wr < H - K && gr + i < a.rows) {                                                                  \
                const ptrdiff_t g = (ptrdiff_t)(gr + i) * a.pitch + gc;                                                      \
                a.out_u[g] = u[i];                                                                                           \
                a.out_v[g] = v[i];                                                                                           \
            }                                                                                                                \
        }                                                                                                                    \
    }
template <int RPW, int FAST>
__global__ __launch_bounds__(kTileWaves * 64) void GS_SUFFIX(gs_ens_tile_k)(GsEnsArgs e, int K, int windows)
{
    GS_ENS_TILE_BODY(RPW, FAST, GS_ENS_MEMBER_OF_GROUP, 0)
}
template <int RPW, int FAST>
__global__ __launch_bounds__(kTileWaves * 64) void GS_SUFFIX(gs_ens_tile_lk)(GsEnsArgs e, const uint32_t *list, int K, int windows)
{
    GS_ENS_TILE_BODY(RPW, FAST, GS_ENS_MEMBER_LISTED, 0)
}
template <int RPW, int FAST>
__global__ __launch_bounds__(kTileWaves * 64) void GS_SUFFIX(gs_ens_tile_zk)(GsEnsArgs e, GsEnsNoiseArgs z, int K, int windows)
{
    GS_ENS_TILE_BODY(RPW, FAST, GS_ENS_MEMBER_NOISE, 1)
}
#undef GS_ENS_TILE_BODY
#undef GS_ENS_TILE_NZ_MEMBER_0
#undef GS_ENS_TILE_NZ_MEMBER_1
#undef GS_ENS_TILE_NZ_T_0
#undef GS_ENS_TILE_NZ_T_1
#undef GS_ENS_TILE_NZ_A_0
#undef GS_ENS_TILE_NZ_A_1

// The periodic rule's windowed form (GsEnsArgs::zero_halo = 2): tile_window_periodic for window `blockIdx.x % windows`
// of member `first + blockIdx.x / windows`; a window wraps around its own member only.
template <int RPW, int FAST>
__global__ __launch_bounds__(kTileWaves * 64) void GS_SUFFIX(gs_ens_tile_pk)(GsEnsArgs e, int K, int windows)
{
    if ((FAST & 1) && !GS_MATH_FUSED) __builtin_amdgcn_s_setreg(1 | (9 << 6), 0); // half_diff: MODE.IEEE = 0
    extern __shared__ float lds[];
    const int m = (int)(blockIdx.x / (unsigned)windows), win = (int)blockIdx.x - m * windows;
    tile_window_periodic<RPW, FAST>(ens_member_args(e, GS_ENS_MEMBER_OF_GROUP(m)), lds, K, win);
}

// The zero-flux rule's windowed form (GsEnsArgs::zero_halo = 3): tile_window_neumann for window `blockIdx.x % windows` of
// member `first + blockIdx.x / windows`.
template <int RPW, int FAST>
__global__ __launch_bounds__(kTileWaves * 64) void GS_SUFFIX(gs_ens_tile_nk)(GsEnsArgs e, int K, int windows)
{
    if ((FAST & 1) && !GS_MATH_FUSED) __builtin_amdgcn_s_setreg(1 | (9 << 6), 0); // half_diff: MODE.IEEE = 0
    extern __shared__ float lds[];
    const int m = (int)(blockIdx.x / (unsigned)windows), win = (int)blockIdx.x - m * windows;
    tile_window_neumann<RPW, FAST>(ens_member_args(e, GS_ENS_MEMBER_OF_GROUP(m)), lds, K, win);
}

// The listed forms of the two: window `blockIdx.x % windows` of member list[first + blockIdx.x / windows].
template <int RPW, int FAST>
__global__ __launch_bounds__(kTileWaves * 64) void GS_SUFFIX(gs_ens_tile_lpk)(GsEnsArgs e, const uint32_t *list, int K, int windows)
{
    if ((FAST & 1) && !GS_MATH_FUSED) __builtin_amdgcn_s_setreg(1 | (9 << 6), 0); // half_diff: MODE.IEEE = 0
    extern __shared__ float lds[];
    const int m = (int)(blockIdx.x / (unsigned)windows), win = (int)blockIdx.x - m * windows;
    tile_window_periodic<RPW, FAST>(ens_member_args(e, GS_ENS_MEMBER_LISTED(m)), lds, K, win);
}
template <int RPW, int FAST>
__global__ __launch_bounds__(kTileWaves * 64) void GS_SUFFIX(gs_ens_tile_lnk)(GsEnsArgs e, const uint32_t *list, int K, int windows)
{
    if ((FAST & 1) && !GS_MATH_FUSED) __builtin_amdgcn_s_setreg(1 | (9 << 6), 0); // half_diff: MODE.IEEE = 0
    extern __shared__ float lds[];
    const int m = (int)(blockIdx.x / (unsigned)windows), win = (int)blockIdx.x - m * windows;
    tile_window_neumann<RPW, FAST>(ens_member_args(e, GS_ENS_MEMBER_LISTED(m)), lds, K, win);
}
// The noise forms of the two: the windows' cells draw at wrapped coordinates under the periodic rule.
template <int RPW, int FAST>
__global__ __launch_bounds__(kTileWaves * 64) void GS_SUFFIX(gs_ens_tile_zpk)(GsEnsArgs e, GsEnsNoiseArgs z, int K, int windows)
{
    if ((FAST & 1) && !GS_MATH_FUSED) __builtin_amdgcn_s_setreg(1 | (9 << 6), 0); // half_diff: MODE.IEEE = 0
    extern __shared__ float lds[];
    const int m = (int)(blockIdx.x / (unsigned)windows), win = (int)blockIdx.x - m * windows;
    const int64_t member = GS_ENS_MEMBER_NOISE(m);
    tile_window_periodic<RPW, FAST, true>(ens_member_args(e, member), lds, K, win, ens_member_noise(z, member));
}
template <int RPW, int FAST>
__global__ __launch_bounds__(kTileWaves * 64) void GS_SUFFIX(gs_ens_tile_znk)(GsEnsArgs e, GsEnsNoiseArgs z, int K, int windows)
{
    if ((FAST & 1) && !GS_MATH_FUSED) __builtin_amdgcn_s_setreg(1 | (9 << 6), 0); // half_diff: MODE.IEEE = 0
    extern __shared__ float lds[];
    const int m = (int)(blockIdx.x / (unsigned)windows), win = (int)blockIdx.x - m * windows;
    const int64_t member = GS_ENS_MEMBER_NOISE(m);
    tile_window_neumann<RPW, FAST, true>(ens_member_args(e, member), lds, K, win, ens_member_noise(z, member));
}
#undef GS_ENS_MEMBER_OF_GROUP
#undef GS_ENS_MEMBER_LISTED
#undef GS_ENS_MEMBER_NOISE

} // namespace
