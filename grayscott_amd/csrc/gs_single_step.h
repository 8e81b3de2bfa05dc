// gs_single_step.h -- one step per launch: the one-thread-per-cell cross-check kernel, the streaming kernel of gs_step
// (HBM-bound: the leg north_star asks the rocprof evidence for) and the LDS-staged alternative.
// Part of the gfx950 step kernels: included by their main unit, gs_step_kernels.hip, behind gs_step_flavour.h (GS_MATH_FUSED,
// GS_SUFFIX, GS_TAP) and gs_cell.h, once per arithmetic flavour; not a header to include elsewhere.
#pragma once

namespace {

// ------------------------------------------------------------------------------------
// Cross-check kernel: literal restatement, one thread per cell.
// ------------------------------------------------------------------------------------
// The reaction of cell (r, c) at plane offset o: the context's rates, or the parameter map's at the cell (MAP, the
// planes of `mp` at the same offset as the cell's U).
template <bool MAP>
__device__ __forceinline__ void simple_react(const GsStepArgs &a, const GsMapPlanes &mp, ptrdiff_t o, float u, float v,
                                             float acc_u, float acc_v, float &ou, float &ov)
{
    if constexpr (MAP)
        react(a, mp.feed[o], mp.fpk[o], u, v, acc_u, acc_v, ou, ov);
    else
        react(a, u, v, acc_u, acc_v, ou, ov);
}

// MASK (the simple kernels' domain-mask forms, gs_step_simple_wk): a tap whose neighbour the cell's link word marks as a wall
// reads the cell's own value (bit (di + 1) * 3 + (dj + 1) for the neighbour at offset (di, dj), after the rule has clamped
// or wrapped it); a wall cell stores its input.
__device__ __forceinline__ bool simple_wall(const GsMaskPlanes &mk, ptrdiff_t o, int bit)
{
    return (reinterpret_cast<const uint32_t *>(mk.link)[o] >> bit) & 1u;
}

template <bool MAP = false, bool MASK = false, bool NOISE = false>
__device__ __forceinline__ void simple_cell(const GsStepArgs &a, const GsMapPlanes &mp = GsMapPlanes{nullptr, nullptr},
                                            const GsMaskPlanes &mk = GsMaskPlanes{nullptr}, const GsNoiseArgs &nz = GsNoiseArgs{})
{
    const int bpr = (a.cols + 255) >> 8;
    const int slot = blockIdx.x / bpr;
    const int c = (blockIdx.x - slot * bpr) * 256 + threadIdx.x;
    const int r = range_row(a, slot);
    if (c >= a.cols) return;

    const bool top = (r > 0) || a.top_present;
    const bool bottom = (r + 1 < a.rows) || a.bottom_present;
    const bool left = c > 0;
    const bool right = c + 1 < a.cols;
    const ptrdiff_t pitch = a.pitch;
    const ptrdiff_t o = (ptrdiff_t)r * pitch + c;
    const float u = a.in_u[o], v = a.in_v[o];

    float acc_u = 0.0f, acc_v = 0.0f;
    if (a.zero_halo) { // full window, centred weights, zeros outside the grid (0 or 1 here: periodic = gs_step_simple_pk)
        for (int di = -1; di <= 1; ++di)
            for (int dj = -1; dj <= 1; ++dj) {
                const bool inside = (di >= 0 || top) && (di <= 0 || bottom) && (dj >= 0 || left) && (dj <= 0 || right);
                float su = inside ? a.in_u[o + di * pitch + dj] : 0.0f;
                float sv = inside ? a.in_v[o + di * pitch + dj] : 0.0f;
                if (MASK && inside && simple_wall(mk, o, (di + 1) * 3 + dj + 1)) { su = u; sv = v; }
                GS_TAP(acc_u, a.w[di + 1][dj + 1], su, u);
                GS_TAP(acc_v, a.w[di + 1][dj + 1], sv, v);
            }
    } else {
        const int i_off = top ? 1 : 0, j_off = left ? 1 : 0;
        for (int di = top ? -1 : 0; di <= (bottom ? 1 : 0); ++di)
            for (int dj = left ? -1 : 0; dj <= (right ? 1 : 0); ++dj) {
                const float w = a.w[di + i_off][dj + j_off];
                float su = a.in_u[o + di * pitch + dj];
                float sv = a.in_v[o + di * pitch + dj];
                if (MASK && simple_wall(mk, o, (di + 1) * 3 + dj + 1)) { su = u; sv = v; }
                GS_TAP(acc_u, w, su, u);
                GS_TAP(acc_v, w, sv, v);
            }
    }
    float ou, ov;
    simple_react<MAP>(a, mp, o, u, v, acc_u, acc_v, ou, ov);
    if (MASK && simple_wall(mk, o, kWallSelf)) { ou = u; ov = v; }
    if constexpr (NOISE) {
        const uint32_t gc[1] = {(uint32_t)c};
        float xu[1] = {ou}, xv[1] = {ov};
        react_noise<1>(nz, nz.key[0], nz.row0 + (uint32_t)r, gc, xu, xv);
        ou = xu[0];
        ov = xv[0];
    }
    a.out_u[o] = ou;
    a.out_v[o] = ov;
}
__global__ __launch_bounds__(256) void GS_SUFFIX(gs_step_simple_k)(GsStepArgs a) { simple_cell(a); }

// The periodic rule (GsStepArgs::zero_halo = 2), literally: the nine taps of the zero-halo rule's interior cell, in its
// order, with neighbour (r + i - 1, c + j - 1) read at ((r + i - 1) mod rows, (c + j - 1) mod cols).  A kernel of its own.
template <bool MAP = false, bool MASK = false, bool NOISE = false>
__device__ __forceinline__ void simple_cell_periodic(const GsStepArgs &a, const GsMapPlanes &mp = GsMapPlanes{nullptr, nullptr},
                                                     const GsMaskPlanes &mk = GsMaskPlanes{nullptr}, const GsNoiseArgs &nz = GsNoiseArgs{})
{
    const int bpr = (a.cols + 255) >> 8;
    const int slot = blockIdx.x / bpr;
    const int c = (blockIdx.x - slot * bpr) * 256 + threadIdx.x;
    const int r = range_row(a, slot);
    if (c >= a.cols) return;
    const ptrdiff_t pitch = a.pitch;
    const ptrdiff_t rows_at[3] = {(ptrdiff_t)(r > 0 ? r - 1 : a.rows - 1) * pitch, (ptrdiff_t)r * pitch,
                                  (ptrdiff_t)(r + 1 < a.rows ? r + 1 : 0) * pitch};
    const int cols_at[3] = {c > 0 ? c - 1 : a.cols - 1, c, c + 1 < a.cols ? c + 1 : 0};
    constexpr bool NEU = false; // MASK: a wrapped neighbour's bit is that of its position
    const float u = a.in_u[rows_at[1] + c], v = a.in_v[rows_at[1] + c];
    float acc_u = 0.0f, acc_v = 0.0f;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            float su = a.in_u[rows_at[i] + cols_at[j]], sv = a.in_v[rows_at[i] + cols_at[j]];
            // (the offset of the cell read, after the rule: a clamped row or column is the cell's own)
            const int ri = rows_at[i] == rows_at[1] ? 1 : i, cj = cols_at[j] == c ? 1 : j;
            if (MASK && !(ri == 1 && cj == 1) && simple_wall(mk, rows_at[1] + c, NEU ? ri * 3 + cj : i * 3 + j)) { su = u; sv = v; }
            GS_TAP(acc_u, a.w[i][j], su, u);
            GS_TAP(acc_v, a.w[i][j], sv, v);
        }
    float ou, ov;
    simple_react<MAP>(a, mp, rows_at[1] + c, u, v, acc_u, acc_v, ou, ov);
    if (MASK && simple_wall(mk, rows_at[1] + c, kWallSelf)) { ou = u; ov = v; }
    if constexpr (NOISE) {
        const uint32_t gc[1] = {(uint32_t)c};
        float xu[1] = {ou}, xv[1] = {ov};
        react_noise<1>(nz, nz.key[0], nz.row0 + (uint32_t)r, gc, xu, xv);
        ou = xu[0];
        ov = xv[0];
    }
    a.out_u[rows_at[1] + c] = ou;
    a.out_v[rows_at[1] + c] = ov;
}
__global__ __launch_bounds__(256) void GS_SUFFIX(gs_step_simple_pk)(GsStepArgs a) { simple_cell_periodic(a); }

// The zero-flux (Neumann) rule (GsStepArgs::zero_halo = 3), literally: the nine taps of the zero-halo rule's interior cell,
// in its order, with neighbour (r + i - 1, c + j - 1) read at the nearest cell of the grid -- rows clamped at the global
// edges only (a slab seam reads its ghost row), columns at 0 and cols - 1.  A kernel of its own.
template <bool MAP = false, bool MASK = false, bool NOISE = false>
__device__ __forceinline__ void simple_cell_neumann(const GsStepArgs &a, const GsMapPlanes &mp = GsMapPlanes{nullptr, nullptr},
                                                    const GsMaskPlanes &mk = GsMaskPlanes{nullptr}, const GsNoiseArgs &nz = GsNoiseArgs{})
{
    const int bpr = (a.cols + 255) >> 8;
    const int slot = blockIdx.x / bpr;
    const int c = (blockIdx.x - slot * bpr) * 256 + threadIdx.x;
    const int r = range_row(a, slot);
    if (c >= a.cols) return;
    const ptrdiff_t pitch = a.pitch;
    const ptrdiff_t rows_at[3] = {(ptrdiff_t)(r > 0 || a.top_present ? r - 1 : r) * pitch, (ptrdiff_t)r * pitch,
                                  (ptrdiff_t)(r + 1 < a.rows || a.bottom_present ? r + 1 : r) * pitch};
    const int cols_at[3] = {c > 0 ? c - 1 : c, c, c + 1 < a.cols ? c + 1 : c};
    constexpr bool NEU = true; // MASK: a clamped neighbour's bit is that of the cell read
    const float u = a.in_u[rows_at[1] + c], v = a.in_v[rows_at[1] + c];
    float acc_u = 0.0f, acc_v = 0.0f;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            float su = a.in_u[rows_at[i] + cols_at[j]], sv = a.in_v[rows_at[i] + cols_at[j]];
            // (the offset of the cell read, after the rule: a clamped row or column is the cell's own)
            const int ri = rows_at[i] == rows_at[1] ? 1 : i, cj = cols_at[j] == c ? 1 : j;
            if (MASK && !(ri == 1 && cj == 1) && simple_wall(mk, rows_at[1] + c, NEU ? ri * 3 + cj : i * 3 + j)) { su = u; sv = v; }
            GS_TAP(acc_u, a.w[i][j], su, u);
            GS_TAP(acc_v, a.w[i][j], sv, v);
        }
    float ou, ov;
    simple_react<MAP>(a, mp, rows_at[1] + c, u, v, acc_u, acc_v, ou, ov);
    if (MASK && simple_wall(mk, rows_at[1] + c, kWallSelf)) { ou = u; ov = v; }
    if constexpr (NOISE) {
        const uint32_t gc[1] = {(uint32_t)c};
        float xu[1] = {ou}, xv[1] = {ov};
        react_noise<1>(nz, nz.key[0], nz.row0 + (uint32_t)r, gc, xu, xv);
        ou = xu[0];
        ov = xv[0];
    }
    a.out_u[rows_at[1] + c] = ou;
    a.out_v[rows_at[1] + c] = ov;
}
__global__ __launch_bounds__(256) void GS_SUFFIX(gs_step_simple_nk)(GsStepArgs a) { simple_cell_neumann(a); }

// The parameter map's form of the three (the planes of GsMapPlanes), the replay check of mapped runs.  RULE = the kernel
// set of the boundary rule: 0 = clipped and zero halo (GsStepArgs::zero_halo read at run time), 1 = periodic, 2 = zero flux.
template <int RULE>
__global__ __launch_bounds__(256) void GS_SUFFIX(gs_step_simple_mk)(GsStepArgs a, GsMapPlanes mp)
{
    if constexpr (RULE == 1) simple_cell_periodic<true>(a, mp);
    else if constexpr (RULE == 2) simple_cell_neumann<true>(a, mp);
    else simple_cell<true>(a, mp);
}
// ... and the domain mask's (the link plane of GsMaskPlanes), the replay check of masked runs.
template <int RULE>
__global__ __launch_bounds__(256) void GS_SUFFIX(gs_step_simple_wk)(GsStepArgs a, GsMaskPlanes mk)
{
    const GsMapPlanes none{nullptr, nullptr};
    if constexpr (RULE == 1) simple_cell_periodic<false, true>(a, none, mk);
    else if constexpr (RULE == 2) simple_cell_neumann<false, true>(a, none, mk);
    else simple_cell<false, true>(a, none, mk);
}

// ... and the noise forms (the keys and sigmas of GsNoiseArgs, gs_ctx_set_noise): the reference cell, then react_noise at
// the cell's global position.
template <int RULE>
__global__ __launch_bounds__(256) void GS_SUFFIX(gs_step_simple_zk)(GsStepArgs a, GsNoiseArgs nz)
{
    const GsMapPlanes none{nullptr, nullptr};
    const GsMaskPlanes nomask{nullptr};
    if constexpr (RULE == 1) simple_cell_periodic<false, false, true>(a, none, nomask, nz);
    else if constexpr (RULE == 2) simple_cell_neumann<false, false, true>(a, none, nomask, nz);
    else simple_cell<false, false, true>(a, none, nomask, nz);
}

// PER: a unit on an edge under the periodic rule (gs_step_stream_pk): rows and columns are read at their index modulo
// the grid's (a lane whose four columns are not one aligned piece of a row after wrapping loads them one by one), and
// every cell runs the interior code.  ZH: the boundary rule of the edge cells (cell<>; -1 = GsStepArgs::zero_halo, 3 = the
// zero-flux rule of gs_step_stream_nk).  MAP: the parameter map's form (gs_step_stream_mk): a cell's rates are read at the
// cell itself -- the rows of the unit, this lane's four columns, the addresses of its stores -- one group ahead, like
// the rows of the species.  MASK: the domain mask's form (gs_step_stream_wk): the link words of the cells, read like MAP's
// rates (in mf), and every cell computed by cell_masked.
// NOISE: the noise form (gs_step_stream_zk): react_noise on every cell computed, at its global row and column.
template <int G, bool EDGE, bool PER = false, int ZH = -1, bool MAP = false, bool MASK = false, bool NOISE = false>
__device__ __forceinline__ void march(const GsStepArgs &a, int ur0, int ur1, int c0, int lane,
                                      const GsMapPlanes &mp = GsMapPlanes{nullptr, nullptr},
                                      const GsMaskPlanes &mkp = GsMaskPlanes{nullptr}, const GsNoiseArgs &nz = GsNoiseArgs{})
{
    const int c = c0 + lane * 4;
    LaneCtx lc;
    lc.lane_ok = !EDGE || (c < a.pitch);
    lc.halo_off = (lane == 0) ? -1 : 4;
    lc.halo_ok = EDGE && !PER ? ((lane == 0 && c0 > 0) || (lane == 63 && c + 4 < a.pitch))
                              : (lane == 0 || lane == 63);

    const ptrdiff_t pitch = a.pitch;
    const float *bu = a.in_u + c, *bv = a.in_v + c; // row 0 of this lane's columns
    float *ou = a.out_u + (ptrdiff_t)ur0 * pitch + c;
    float *ov = a.out_v + (ptrdiff_t)ur0 * pitch + c;

    // Rows are fetched one group (G rows) ahead of the group being computed.  Row indices
    // are clamped to ur1 (the row below the last output row, at most the bottom ghost
    // row), so every load is in bounds and the tail needs no branches around loads.
    // PER: this lane's first column and its halo column modulo the grid's columns
    int pc0 = 0, phalo = 0;
    bool pvec = true;
    if constexpr (PER) {
        pc0 = c % a.cols;
        pvec = pc0 % 4 == 0 && pc0 + 4 <= a.cols;
        phalo = (lane == 0 ? c0 - 1 + a.cols : c + 4) % a.cols;
    }
    auto fetch = [&](int row) {
        const int rr = row < ur1 ? row : ur1;
        if constexpr (PER) {
            const int wr = rr < 0 ? rr + a.rows : (rr >= a.rows ? rr - a.rows : rr); // |rr| stays within a row of the grid
            const float *pu = a.in_u + (ptrdiff_t)wr * pitch, *pv = a.in_v + (ptrdiff_t)wr * pitch;
            RowIn r;
            if (pvec) {
                r.u = *reinterpret_cast<const float4 *>(pu + pc0);
                r.v = *reinterpret_cast<const float4 *>(pv + pc0);
            } else {
                float xu[4], xv[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    int cc = pc0 + i;
                    if (cc >= a.cols) cc -= a.cols;
                    if (cc >= a.cols) cc %= a.cols;
                    xu[i] = pu[cc];
                    xv[i] = pv[cc];
                }
                r.u = make_float4(xu[0], xu[1], xu[2], xu[3]);
                r.v = make_float4(xv[0], xv[1], xv[2], xv[3]);
            }
            r.hu = 0.f;
            r.hv = 0.f;
            if (lc.halo_ok) {
                r.hu = pu[phalo];
                r.hv = pv[phalo];
            }
            return r;
        }
        return load_row<EDGE>(bu + (ptrdiff_t)rr * pitch, bv + (ptrdiff_t)rr * pitch, lc);
    };

    // MAP: (F, F + K) of this lane's four cells of `row` (rows past ur1 are not computed: clamped like fetch's)
    auto fetch_rates = [&](int row, float4 &f, float4 &fk) {
        const ptrdiff_t o = (ptrdiff_t)(row < ur1 ? row : ur1 - 1) * pitch + c;
        f = make_float4(0.f, 0.f, 0.f, 0.f);
        fk = f;
        if (lc.lane_ok) {
            if constexpr (MASK) {
                f = *reinterpret_cast<const float4 *>(mkp.link + o);
            } else {
                f = *reinterpret_cast<const float4 *>(mp.feed + o);
                fk = *reinterpret_cast<const float4 *>(mp.fpk + o);
            }
        }
    };

    RowW q[G + 2];
    RowIn n[G];
    float4 mf[G] = {}, mk[G] = {}; // MAP: the rates of the group being computed
    q[0] = widen(fetch(ur0 - 1));
    q[1] = widen(fetch(ur0));
#pragma unroll
    for (int g = 0; g < G; ++g) n[g] = fetch(ur0 + 1 + g);
    if constexpr (MAP || MASK) {
#pragma unroll
        for (int g = 0; g < G; ++g) fetch_rates(ur0 + g, mf[g], mk[g]);
    }

    // per-lane masks (all ones = that neighbour column is clipped away).  c is a multiple of 4,
    // so only the first of a lane's four cells can sit on the global left edge.
    uint32_t la[4], ra[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        la[k] = (EDGE && k == 0 && c == 0) ? 0xffffffffu : 0u;
        ra[k] = (EDGE && (c + k + 1 >= a.cols)) ? 0xffffffffu : 0u;
        if (EDGE && !PER) { // keep the masks opaque, or the compiler turns every blend back into v_cndmask
            if (k == 0) asm volatile("" : "+v"(la[k]));
            asm volatile("" : "+v"(ra[k]));
        }
    }

    for (int r = ur0; r < ur1; r += G) {
#pragma unroll
        for (int g = 0; g < G; ++g) q[g + 2] = widen(n[g]);
#pragma unroll
        for (int g = 0; g < G; ++g) n[g] = fetch(r + G + 1 + g);
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int row = r + g;
            if (row < ur1) {
                const bool mrow = !EDGE || (row > 0) || a.top_present;
                const bool prow = !EDGE || (row + 1 < a.rows) || a.bottom_present;
                float4 nu, nv;
                constexpr bool E = EDGE && !PER;
                if constexpr (MASK) {
                    auto w = [](float x) { return __builtin_bit_cast(uint32_t, x); };
                    cell_masked<E, 0, RowW, ZH>(a, q[g], q[g + 1], q[g + 2], 1, mrow, prow, la[0], ra[0], w(mf[g].x), nu.x, nv.x);
                    cell_masked<E, 0, RowW, ZH>(a, q[g], q[g + 1], q[g + 2], 2, mrow, prow, la[1], ra[1], w(mf[g].y), nu.y, nv.y);
                    cell_masked<E, 0, RowW, ZH>(a, q[g], q[g + 1], q[g + 2], 3, mrow, prow, la[2], ra[2], w(mf[g].z), nu.z, nv.z);
                    cell_masked<E, 0, RowW, ZH>(a, q[g], q[g + 1], q[g + 2], 4, mrow, prow, la[3], ra[3], w(mf[g].w), nu.w, nv.w);
                } else {
                    cell<E, 0, RowW, ZH, MAP>(a, q[g], q[g + 1], q[g + 2], 1, mrow, prow, la[0], ra[0], nu.x, nv.x, mf[g].x, mk[g].x);
                    cell<E, 0, RowW, ZH, MAP>(a, q[g], q[g + 1], q[g + 2], 2, mrow, prow, la[1], ra[1], nu.y, nv.y, mf[g].y, mk[g].y);
                    cell<E, 0, RowW, ZH, MAP>(a, q[g], q[g + 1], q[g + 2], 3, mrow, prow, la[2], ra[2], nu.z, nv.z, mf[g].z, mk[g].z);
                    cell<E, 0, RowW, ZH, MAP>(a, q[g], q[g + 1], q[g + 2], 4, mrow, prow, la[3], ra[3], nu.w, nv.w, mf[g].w, mk[g].w);
                }
                if constexpr (NOISE) {
                    const uint32_t gc[4] = {(uint32_t)c, (uint32_t)c + 1u, (uint32_t)c + 2u, (uint32_t)c + 3u};
                    float xu[4] = {nu.x, nu.y, nu.z, nu.w}, xv[4] = {nv.x, nv.y, nv.z, nv.w};
                    react_noise<4>(nz, nz.key[0], nz.row0 + (uint32_t)row, gc, xu, xv);
                    nu = make_float4(xu[0], xu[1], xu[2], xu[3]);
                    nv = make_float4(xv[0], xv[1], xv[2], xv[3]);
                }
                if (lc.lane_ok) {
                    *reinterpret_cast<float4 *>(ou) = nu;
                    *reinterpret_cast<float4 *>(ov) = nv;
                }
                ou += pitch;
                ov += pitch;
            }
        }
        q[0] = q[G];
        q[1] = q[G + 1];
        if constexpr (MAP || MASK) {
#pragma unroll
            for (int g = 0; g < G; ++g) fetch_rates(r + G + g, mf[g], mk[g]);
        }
    }
}

template <int G>
__global__ __launch_bounds__(256) void GS_SUFFIX(gs_step_stream_k)(GsStepArgs a)
{
    const int lane = threadIdx.x & 63;
    // readfirstlane tells the compiler the wave index is wave-uniform: everything derived
    // from it (unit, row range, edge flags) then lives in SGPRs and branches are scalar.
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int strips = (a.cols + 255) >> 8;
    int block = (int)blockIdx.x;
    if (a.xcd_m > 0) { // XCD-aware order (GsStepArgs::xcd_m)
        const int per = 8 * a.xcd_m, g = block / per, o = block - g * per;
        if ((g + 1) * per <= (int)gridDim.x) block = g * per + (o & 7) * a.xcd_m + (o >> 3);
    }
    const int unit = block * 4 + wave;
    const int chunk = unit / strips;
    const int strip = unit - chunk * strips;
    const int rpu = a.rows_per_unit;
    const int chunks_a = (a.ra1 - a.ra0 + rpu - 1) / rpu;
    const int chunks_b = (a.rb1 - a.rb0 + rpu - 1) / rpu;
    if (chunk >= chunks_a + chunks_b) return; // wave-uniform

    int ur0, ur1;
    if (chunk < chunks_a) {
        ur0 = a.ra0 + chunk * rpu;
        ur1 = min(ur0 + rpu, a.ra1);
    } else {
        ur0 = a.rb0 + (chunk - chunks_a) * rpu;
        ur1 = min(ur0 + rpu, a.rb1);
    }
    const int c0 = strip << 8;
    // Units that touch a global edge or the ragged right end take the general path; the
    // interior path has no per-lane bounds logic at all.
    const bool edge = (c0 == 0) || (c0 + 256 >= a.cols) || (ur0 == 0 && !a.top_present) ||
                      (ur1 == a.rows && !a.bottom_present);
    if (edge)
        march<G, true>(a, ur0, ur1, c0, lane);
    else
        march<G, false>(a, ur0, ur1, c0, lane);
}

// The periodic rule's form (GsStepArgs::zero_halo = 2; a single slab): gs_step_stream_k's units, whose
// edge units read wrapped rows and columns and run the interior cell code (march<PER>).
template <int G>
__global__ __launch_bounds__(256) void GS_SUFFIX(gs_step_stream_pk)(GsStepArgs a)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int strips = (a.cols + 255) >> 8;
    int block = (int)blockIdx.x;
    if (a.xcd_m > 0) { // XCD-aware order (GsStepArgs::xcd_m)
        const int per = 8 * a.xcd_m, g = block / per, o = block - g * per;
        if ((g + 1) * per <= (int)gridDim.x) block = g * per + (o & 7) * a.xcd_m + (o >> 3);
    }
    const int unit = block * 4 + wave;
    const int chunk = unit / strips;
    const int strip = unit - chunk * strips;
    const int rpu = a.rows_per_unit;
    const int chunks_a = (a.ra1 - a.ra0 + rpu - 1) / rpu;
    const int chunks_b = (a.rb1 - a.rb0 + rpu - 1) / rpu;
    if (chunk >= chunks_a + chunks_b) return; // wave-uniform
    int ur0, ur1;
    if (chunk < chunks_a) {
        ur0 = a.ra0 + chunk * rpu;
        ur1 = min(ur0 + rpu, a.ra1);
    } else {
        ur0 = a.rb0 + (chunk - chunks_a) * rpu;
        ur1 = min(ur0 + rpu, a.rb1);
    }
    const int c0 = strip << 8;
    const bool edge = (c0 == 0) || (c0 + 256 >= a.cols) || (ur0 == 0) || (ur1 == a.rows);
    if (edge)
        march<G, true, true>(a, ur0, ur1, c0, lane);
    else
        march<G, false>(a, ur0, ur1, c0, lane);
}

// The zero-flux rule's form (GsStepArgs::zero_halo = 3): gs_step_stream_k's units, whose edge units run the rule's edge
// cell (cell<ZH = 3>: the missing row / column is the cell's own); slab seams read their ghost rows as in gs_step_stream_k.
template <int G>
__global__ __launch_bounds__(256) void GS_SUFFIX(gs_step_stream_nk)(GsStepArgs a)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int strips = (a.cols + 255) >> 8;
    int block = (int)blockIdx.x;
    if (a.xcd_m > 0) { // XCD-aware order (GsStepArgs::xcd_m)
        const int per = 8 * a.xcd_m, g = block / per, o = block - g * per;
        if ((g + 1) * per <= (int)gridDim.x) block = g * per + (o & 7) * a.xcd_m + (o >> 3);
    }
    const int unit = block * 4 + wave;
    const int chunk = unit / strips;
    const int strip = unit - chunk * strips;
    const int rpu = a.rows_per_unit;
    const int chunks_a = (a.ra1 - a.ra0 + rpu - 1) / rpu;
    const int chunks_b = (a.rb1 - a.rb0 + rpu - 1) / rpu;
    if (chunk >= chunks_a + chunks_b) return; // wave-uniform
    int ur0, ur1;
    if (chunk < chunks_a) {
        ur0 = a.ra0 + chunk * rpu;
        ur1 = min(ur0 + rpu, a.ra1);
    } else {
        ur0 = a.rb0 + (chunk - chunks_a) * rpu;
        ur1 = min(ur0 + rpu, a.rb1);
    }
    const int c0 = strip << 8;
    const bool edge = (c0 == 0) || (c0 + 256 >= a.cols) || (ur0 == 0 && !a.top_present) ||
                      (ur1 == a.rows && !a.bottom_present);
    if (edge)
        march<G, true, false, 3>(a, ur0, ur1, c0, lane);
    else
        march<G, false>(a, ur0, ur1, c0, lane);
}

// The parameter map's form of the three (the planes of GsMapPlanes): their units, edge tests and marches, with the map's
// rates.  RULE = the kernel set of the boundary rule: 0 = clipped and zero halo, 1 = periodic, 2 = zero flux.
template <int G, int RULE>
__global__ __launch_bounds__(256) void GS_SUFFIX(gs_step_stream_mk)(GsStepArgs a, GsMapPlanes mp)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int strips = (a.cols + 255) >> 8;
    int block = (int)blockIdx.x;
    if (a.xcd_m > 0) { // XCD-aware order (GsStepArgs::xcd_m)
        const int per = 8 * a.xcd_m, g = block / per, o = block - g * per;
        if ((g + 1) * per <= (int)gridDim.x) block = g * per + (o & 7) * a.xcd_m + (o >> 3);
    }
    const int unit = block * 4 + wave;
    const int chunk = unit / strips;
    const int strip = unit - chunk * strips;
    const int rpu = a.rows_per_unit;
    const int chunks_a = (a.ra1 - a.ra0 + rpu - 1) / rpu;
    const int chunks_b = (a.rb1 - a.rb0 + rpu - 1) / rpu;
    if (chunk >= chunks_a + chunks_b) return; // wave-uniform
    int ur0, ur1;
    if (chunk < chunks_a) {
        ur0 = a.ra0 + chunk * rpu;
        ur1 = min(ur0 + rpu, a.ra1);
    } else {
        ur0 = a.rb0 + (chunk - chunks_a) * rpu;
        ur1 = min(ur0 + rpu, a.rb1);
    }
    const int c0 = strip << 8;
    const bool edge = (c0 == 0) || (c0 + 256 >= a.cols) || (ur0 == 0 && !a.top_present) ||
                      (ur1 == a.rows && !a.bottom_present);
    if (!edge)
        march<G, false, false, -1, true>(a, ur0, ur1, c0, lane, mp);
    else if constexpr (RULE == 1)
        march<G, true, true, -1, true>(a, ur0, ur1, c0, lane, mp);
    else if constexpr (RULE == 2)
        march<G, true, false, 3, true>(a, ur0, ur1, c0, lane, mp);
    else
        march<G, true, false, -1, true>(a, ur0, ur1, c0, lane, mp);
}

// ... and the domain mask's (the link plane of GsMaskPlanes): the same units, every cell through cell_masked.
template <int G, int RULE>
__global__ __launch_bounds__(256) void GS_SUFFIX(gs_step_stream_wk)(GsStepArgs a, GsMaskPlanes mk)
{
    const GsMapPlanes none{nullptr, nullptr};
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int strips = (a.cols + 255) >> 8;
    int block = (int)blockIdx.x;
    if (a.xcd_m > 0) { // XCD-aware order (GsStepArgs::xcd_m)
        const int per = 8 * a.xcd_m, g = block / per, o = block - g * per;
        if ((g + 1) * per <= (int)gridDim.x) block = g * per + (o & 7) * a.xcd_m + (o >> 3);
    }
    const int unit = block * 4 + wave;
    const int chunk = unit / strips;
    const int strip = unit - chunk * strips;
    const int rpu = a.rows_per_unit;
    const int chunks_a = (a.ra1 - a.ra0 + rpu - 1) / rpu;
    const int chunks_b = (a.rb1 - a.rb0 + rpu - 1) / rpu;
    if (chunk >= chunks_a + chunks_b) return; // wave-uniform
    int ur0, ur1;
    if (chunk < chunks_a) {
        ur0 = a.ra0 + chunk * rpu;
        ur1 = min(ur0 + rpu, a.ra1);
    } else {
        ur0 = a.rb0 + (chunk - chunks_a) * rpu;
        ur1 = min(ur0 + rpu, a.rb1);
    }
    const int c0 = strip << 8;
    const bool edge = (c0 == 0) || (c0 + 256 >= a.cols) || (ur0 == 0 && !a.top_present) ||
                      (ur1 == a.rows && !a.bottom_present);
    if (!edge)
        march<G, false, false, -1, false, true>(a, ur0, ur1, c0, lane, none, mk);
    else if constexpr (RULE == 1)
        march<G, true, true, -1, false, true>(a, ur0, ur1, c0, lane, none, mk);
    else if constexpr (RULE == 2)
        march<G, true, false, 3, false, true>(a, ur0, ur1, c0, lane, none, mk);
    else
        march<G, true, false, -1, false, true>(a, ur0, ur1, c0, lane, none, mk);
}

// ... and the noise forms (GsNoiseArgs): the same units, react_noise behind every cell.
template <int G, int RULE>
__global__ __launch_bounds__(256) void GS_SUFFIX(gs_step_stream_zk)(GsStepArgs a, GsNoiseArgs nz)
{
    const GsMapPlanes none{nullptr, nullptr};
    const GsMaskPlanes nomask{nullptr};
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int strips = (a.cols + 255) >> 8;
    int block = (int)blockIdx.x;
    if (a.xcd_m > 0) { // XCD-aware order (GsStepArgs::xcd_m)
        const int per = 8 * a.xcd_m, g = block / per, o = block - g * per;
        if ((g + 1) * per <= (int)gridDim.x) block = g * per + (o & 7) * a.xcd_m + (o >> 3);
    }
    const int unit = block * 4 + wave;
    const int chunk = unit / strips;
    const int strip = unit - chunk * strips;
    const int rpu = a.rows_per_unit;
    const int chunks_a = (a.ra1 - a.ra0 + rpu - 1) / rpu;
    const int chunks_b = (a.rb1 - a.rb0 + rpu - 1) / rpu;
    if (chunk >= chunks_a + chunks_b) return; // wave-uniform
    int ur0, ur1;
    if (chunk < chunks_a) {
        ur0 = a.ra0 + chunk * rpu;
        ur1 = min(ur0 + rpu, a.ra1);
    } else {
        ur0 = a.rb0 + (chunk - chunks_a) * rpu;
        ur1 = min(ur0 + rpu, a.rb1);
    }
    const int c0 = strip << 8;
    const bool edge = (c0 == 0) || (c0 + 256 >= a.cols) || (ur0 == 0 && !a.top_present) ||
                      (ur1 == a.rows && !a.bottom_present);
    if (!edge)
        march<G, false, false, -1, false, false, true>(a, ur0, ur1, c0, lane, none, nomask, nz);
    else if constexpr (RULE == 1)
        march<G, true, true, -1, false, false, true>(a, ur0, ur1, c0, lane, none, nomask, nz);
    else if constexpr (RULE == 2)
        march<G, true, false, 3, false, false, true>(a, ur0, ur1, c0, lane, none, nomask, nz);
    else
        march<G, true, false, -1, false, false, true>(a, ur0, ur1, c0, lane, none, nomask, nz);
}

// ------------------------------------------------------------------------------------
// LDS-staged variant (one step per launch): the (tile + halo) stencil window of a block is
// staged in LDS, then every lane reads its 3 x 6 neighbourhood back with ds_read_b128 +
// two ds_read_b32 per row and species.  Kept as a measured alternative to the register
// sliding window of gs_step_stream_k (north_star names LDS staging explicitly): it moves the
// same HBM bytes, but adds an LDS write + read pass and a barrier per tile, and loses the
// row-to-row register reuse (each input row is read from LDS three times).  Slower than the
// stream kernel on MI355X, so GS_KERNEL_AUTO never picks it.
// ------------------------------------------------------------------------------------
constexpr int kLdsTileRows = 16;          // output rows per block (38 KB of LDS -> 4 blocks per CU)
constexpr int kLdsRowFloats = 256 + 8;    // 4 halo floats each side keep float4 alignment

template <bool EDGE>
__device__ __forceinline__ void lds_tile(const GsStepArgs &a, int tr0, int tr1, int c0, float *su, float *sv)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = c0 + lane * 4;
    const ptrdiff_t pitch = a.pitch;
    const bool lane_ok = !EDGE || (c < a.pitch);
    const bool halo_l = (lane == 0) && (!EDGE || c0 > 0);
    const bool halo_r = (lane == 63) && (!EDGE || c + 4 < a.pitch);
    // stage rows [tr0 - 1, tr1 + 1) of both species; row r lands in LDS row (r - tr0 + 1)
    const int nrows = tr1 - tr0 + 2;
    for (int lr = wave; lr < nrows; lr += 4) {
        const int r = tr0 - 1 + lr; // ghost rows exist physically, so every row is loadable
        float4 fu = make_float4(0.f, 0.f, 0.f, 0.f), fv = fu;
        if (lane_ok) {
            fu = *reinterpret_cast<const float4 *>(a.in_u + (ptrdiff_t)r * pitch + c);
            fv = *reinterpret_cast<const float4 *>(a.in_v + (ptrdiff_t)r * pitch + c);
        }
        float *du = su + lr * kLdsRowFloats + 4 + lane * 4;
        float *dv = sv + lr * kLdsRowFloats + 4 + lane * 4;
        *reinterpret_cast<float4 *>(du) = fu;
        *reinterpret_cast<float4 *>(dv) = fv;
        if (halo_l) {
            du[-1] = a.in_u[(ptrdiff_t)r * pitch + c - 1];
            dv[-1] = a.in_v[(ptrdiff_t)r * pitch + c - 1];
        }
        if (halo_r) {
            du[4] = a.in_u[(ptrdiff_t)r * pitch + c + 4];
            dv[4] = a.in_v[(ptrdiff_t)r * pitch + c + 4];
        }
    }
    __syncthreads();

    // per-lane masks (all ones = that neighbour column is clipped away).  c is a multiple of 4,
    // so only the first of a lane's four cells can sit on the global left edge.
    uint32_t la[4], ra[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        la[k] = (EDGE && k == 0 && c == 0) ? 0xffffffffu : 0u;
        ra[k] = (EDGE && (c + k + 1 >= a.cols)) ? 0xffffffffu : 0u;
        if (EDGE) { // keep the masks opaque, or the compiler turns every blend back into v_cndmask
            if (k == 0) asm volatile("" : "+v"(la[k]));
            asm volatile("" : "+v"(ra[k]));
        }
    }
    auto read_row = [&](int lr) {
        RowW w;
        const float *pu = su + lr * kLdsRowFloats + 4 + lane * 4;
        const float *pv = sv + lr * kLdsRowFloats + 4 + lane * 4;
        const float4 fu = *reinterpret_cast<const float4 *>(pu);
        const float4 fv = *reinterpret_cast<const float4 *>(pv);
        w.u[1] = fu.x; w.u[2] = fu.y; w.u[3] = fu.z; w.u[4] = fu.w;
        w.v[1] = fv.x; w.v[2] = fv.y; w.v[3] = fv.z; w.v[4] = fv.w;
        w.u[0] = pu[-1]; w.u[5] = pu[4];
        w.v[0] = pv[-1]; w.v[5] = pv[4];
        return w;
    };
    for (int r = tr0 + wave; r < tr1; r += 4) {
        const int lr = r - tr0 + 1;
        const RowW m = read_row(lr - 1), z = read_row(lr), p = read_row(lr + 1);
        const bool mrow = !EDGE || (r > 0) || a.top_present;
        const bool prow = !EDGE || (r + 1 < a.rows) || a.bottom_present;
        float4 nu, nv;
        cell<EDGE>(a, m, z, p, 1, mrow, prow, la[0], ra[0], nu.x, nv.x);
        cell<EDGE>(a, m, z, p, 2, mrow, prow, la[1], ra[1], nu.y, nv.y);
        cell<EDGE>(a, m, z, p, 3, mrow, prow, la[2], ra[2], nu.z, nv.z);
        cell<EDGE>(a, m, z, p, 4, mrow, prow, la[3], ra[3], nu.w, nv.w);
        if (lane_ok) {
            *reinterpret_cast<float4 *>(a.out_u + (ptrdiff_t)r * pitch + c) = nu;
            *reinterpret_cast<float4 *>(a.out_v + (ptrdiff_t)r * pitch + c) = nv;
        }
    }
}

__global__ __launch_bounds__(256) void GS_SUFFIX(gs_step_lds_k)(GsStepArgs a)
{
    __shared__ __attribute__((aligned(16))) float su[(kLdsTileRows + 2) * kLdsRowFloats];
    __shared__ __attribute__((aligned(16))) float sv[(kLdsTileRows + 2) * kLdsRowFloats];
    const int strips = (a.cols + 255) >> 8;
    const int chunk = blockIdx.x / strips;
    const int strip = blockIdx.x - chunk * strips;
    const int chunks_a = (a.ra1 - a.ra0 + kLdsTileRows - 1) / kLdsTileRows;
    int tr0, tr1;
    if (chunk < chunks_a) {
        tr0 = a.ra0 + chunk * kLdsTileRows;
        tr1 = min(tr0 + kLdsTileRows, a.ra1);
    } else {
        tr0 = a.rb0 + (chunk - chunks_a) * kLdsTileRows;
        tr1 = min(tr0 + kLdsTileRows, a.rb1);
    }
    const int c0 = strip << 8;
    const bool edge = (c0 == 0) || (c0 + 256 >= a.cols) || (tr0 == 0 && !a.top_present) ||
                      (tr1 == a.rows && !a.bottom_present);
    if (edge)
        lds_tile<true>(a, tr0, tr1, c0, su, sv);
    else
        lds_tile<false>(a, tr0, tr1, c0, su, sv);
}

} // namespace
