// bm_sort.h — the build's stable radix sort of (key, value) pairs: digit histograms, one-sweep passes with
// decoupled look-back, the top-digit-first bucket sort and its plan, and the host-side pass launcher.
// Included by bm_build.hip only, inside its `namespace bm { namespace {`, after the metadata layout
// (RADIX, META_*), BLOCK, blocks_for and bm_bdiag.h: the kernels stay in that translation unit.
// RecJob / gather_records (the triangle records and corner normals gathered by extra workgroups of the
// top-digit pass) live here with k_onesweep_wide, which runs them: launch_build only fills in a RecJob.

// look-back word: flag in the top two bits, count below (counts < MAX_TRIS = 2^27)
constexpr uint32_t LB_AGG = 1u << 30;   // the tile's own digit count
constexpr uint32_t LB_PRE = 2u << 30;   // inclusive digit count over tiles 0..this
constexpr uint32_t LB_MASK = LB_AGG - 1;
// bucket plan words (bucket_plan): order, starts, skew flag
constexpr uint32_t PLAN_ORDER = 0, PLAN_START = RADIX, PLAN_FLAG = 2 * RADIX, PLAN_WORDS = 2 * RADIX + 1;
constexpr int LB_WIN = 8;  // predecessor words fetched per look-back step (on_tile)

// ---- ranked top digit (reference-mode pair sort) ------------------------------------------------------
// The reference's leaf paths are 31-bit keys: four 10-bit passes, the last over one bit. Their top 11 bits
// (the path's first 11 levels) take few values for a scene inside the reference's +-30 world — the
// (leaf, face) pairs of the bunny fall in 8 of the 2,048 — and the count pass marks the values present
// in a 2,048-bit map (`topmap`). The sort then runs three passes: bits 0-9, 10-19, and the rank of bits
// 20-30 among the values present (order-preserving, < 1,024 when at most 1,024 are present: the host
// checks). The keys themselves are not changed, so the sorted output is the four-pass one.
constexpr uint32_t TOP_BITS = 11, TOP_VALUES = 1u << TOP_BITS, TOPMAP_WORDS = TOP_VALUES / 32;
constexpr int TOP_SHIFT = 31 - (int)TOP_BITS;  // 20: the 11 bits above the two low digits of a 31-bit key
template <bool RANK>
__device__ __forceinline__ uint32_t sort_digit(uint32_t key, int shift, const uint16_t* srank) {
    return RANK ? (uint32_t)srank[key >> TOP_SHIFT] : (key >> shift) & (RADIX - 1);
}
// srank[v] = number of present values below v, from the map; one barrier inside (all threads call it)
__device__ void build_top_rank(const uint32_t* __restrict__ topmap, uint16_t* srank, uint32_t* swpre, uint32_t nthreads) {
    const uint32_t t = threadIdx.x;
    if (t < 64) {
        const uint32_t c = t < TOPMAP_WORDS ? (uint32_t)__popc(topmap[t]) : 0u;
        uint32_t incl = c;  // inclusive prefix over the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = (uint32_t)__shfl_up((int)incl, o);
            if ((int)t >= o) incl += y;
        }
        swpre[t] = incl - c;
    }
    __syncthreads();
    for (uint32_t v = t; v < TOP_VALUES; v += nthreads) {
        const uint32_t w = topmap[v >> 5];
        srank[v] = (uint16_t)(swpre[v >> 5] + (uint32_t)__popc(w & ((1u << (v & 31)) - 1u)));
    }
}

// Digit histograms of every pass of a generic key sort (k_morton fuses this for the BVH build). topmap:
// the last pass (2) histograms ranked top digits (see build_top_rank).
constexpr int DH_ITEMS = 16, DH_TILE = BLOCK * DH_ITEMS;  // keys per thread, per workgroup of k_digit_hist
__global__ __launch_bounds__(BLOCK) void k_digit_hist(const uint32_t* __restrict__ keys, uint32_t n, int passes,
                                                      uint32_t* __restrict__ smeta,
                                                      const uint32_t* __restrict__ topmap) {
    __shared__ uint32_t h[4 * RADIX];
    __shared__ uint16_t srank[TOP_VALUES];
    __shared__ uint32_t swpre[64];
    for (uint32_t d = threadIdx.x; d < 4 * RADIX; d += BLOCK) h[d] = 0;
    if (topmap) build_top_rank(topmap, srank, swpre, BLOCK);
    __syncthreads();
    const uint32_t base = blockIdx.x * DH_TILE;
    uint32_t kk[DH_ITEMS];
#pragma unroll
    for (int it = 0; it < DH_ITEMS; ++it) kk[it] = keys[min(base + it * BLOCK + threadIdx.x, n - 1)];
    // A digit the whole wave shares (the high digits of spatially ordered keys: a reference-mode pair
    // list's top path bits) is one LDS add of the wave's count instead of 64 conflicting ones.
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (int it = 0; it < DH_ITEMS; ++it) {
        const bool valid = base + it * BLOCK + threadIdx.x < n;
        const unsigned long long vm = ballot(valid);
        if (!vm) break;
        for (int p = 0; p < passes; ++p) {
            const uint32_t d = (topmap && p == 2) ? sort_digit<true>(kk[it], 0, srank)
                                                  : sort_digit<false>(kk[it], p * RADIX_BITS, nullptr);
            const uint32_t d0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)d);
            if ((ballot(d == d0) & vm) == vm) {
                if (lane == 0) atomicAdd(&h[p * RADIX + d0], (uint32_t)__popcll(vm));
            } else if (valid) {
                atomicAdd(&h[p * RADIX + d], 1u);
            }
        }
    }
    __syncthreads();
    for (uint32_t d = threadIdx.x; d < (uint32_t)passes * RADIX; d += BLOCK)
        if (h[d]) atomicAdd(&smeta[4 + d], h[d]);
}

__device__ __forceinline__ uint32_t lb_load(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void lb_store(uint32_t* p, uint32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Words handed between phases of one launch (C = true: the LSD fallback's two passes in one launch) go
// through device-coherent accesses (global_load/store sc1: written through and read past the per-XCD
// L2s), and a phase is published by its workgroup waiting for its own stores and then counting itself
// done (coh_done) — no agent-scope release fence, whose L2 write-back (buffer_wbl2) per workgroup
// serialised such hand-offs at ~0.4 us each (measured with a fused chunk + table + record kernel,
// DESIGN.md §4). C = false: plain accesses.
template <bool C, class T>
__device__ __forceinline__ T cld(const T* p) {
    static_assert(sizeof(T) == 4, "32-bit words");
    if constexpr (C) return __hip_atomic_load(const_cast<T*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else return *p;
}
template <bool C, class T>
__device__ __forceinline__ void cst(T* p, T v) {
    static_assert(sizeof(T) == 4, "32-bit words");
    if constexpr (C) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *p = v;
}
// Every store of this workgroup (device-coherent ones included) complete, then one count on ctr.
__device__ __forceinline__ void coh_done(uint32_t* ctr) {
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// Wait for `want` counts on ctr. Only workgroups with smaller tickets are awaited (running or done).
__device__ __forceinline__ void coh_wait(const uint32_t* ctr, uint32_t want) {
    if (threadIdx.x == 0)
        while (__hip_atomic_load(const_cast<uint32_t*>(ctr), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < want)
            __builtin_amdgcn_s_sleep(8);
    __syncthreads();
}

// One pass of the one-sweep stable radix sort (Adinets & Merrill 2022 style): each workgroup takes
// the next tile by ticket, publishes its digit counts, resolves its per-digit offset among earlier
// tiles by decoupled look-back, and scatters. A tile only waits on tiles with smaller tickets, which
// are already running and publish their counts without waiting, so the look-back always ends.
// Within a tile each wave ranks its own contiguous chunk (RADIX_BITS 64-lane ballots + per-wave
// running digit counts), then one pass over the digits turns the per-wave counts into offsets:
// two barriers per tile, and the sort is stable — its output is the unique stable order of the keys.
// smeta: the sort's metadata block (sort_meta_words), zero-filled: [0, 4) tickets, [4, 4 + passes *
// RADIX) digit histograms, then the per-pass look-back words.
// One tile (ticket vid) of a one-sweep pass with BLOCK lanes (four digits per thread); LDS from the
// caller (k_bucket_sort<256>, which runs the LSD fallback's last pass with it). lbs: tiles per pass in
// the look-back area (its stride).
template <int ITEMS>
__device__ __forceinline__ void on_tile(uint32_t* __restrict__ wc, uint32_t* __restrict__ running,
                                        uint32_t* __restrict__ wsum, const uint32_t* __restrict__ kin,
                                        const uint32_t* __restrict__ vin, uint32_t* __restrict__ kout,
                                        uint32_t* __restrict__ vout, uint32_t n, int pass, int passes,
                                        uint32_t* __restrict__ smeta, uint32_t lbs, uint32_t vid) {
    const int t = threadIdx.x, w = t >> 6, lane = t & 63;
    for (uint32_t d = t; d < RADIX; d += BLOCK) {
        running[d] = 0;
#pragma unroll
        for (int q = 0; q < BLOCK / 64; ++q) wc[q * RADIX + d] = 0;
    }
    __syncthreads();
    const uint32_t base = vid * (BLOCK * ITEMS);
    const int shift = pass * RADIX_BITS;
    uint32_t k[ITEMS], v[ITEMS];
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {  // each wave: a contiguous chunk of the tile (stability)
        const uint32_t i = min(base + w * (64 * ITEMS) + it * 64 + lane, n - 1);  // branch-free: one latency
        k[it] = kin[i];
        v[it] = vin[i];
    }
#pragma unroll
    for (int it = 0; it < ITEMS; ++it)
        if (base + w * (64 * ITEMS) + it * 64 + lane < n) atomicAdd(&running[(k[it] >> shift) & (RADIX - 1)], 1u);
    __syncthreads();
    // this thread owns digits 4t..4t+3: publish the tile's counts, then resolve their offsets
    uint32_t* lb = smeta + 4 + (size_t)passes * RADIX + (size_t)pass * lbs * RADIX;
    uint32_t cnt[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        cnt[j] = running[4 * t + j];
        lb_store(&lb[(size_t)vid * RADIX + 4 * t + j], (vid == 0 ? LB_PRE : LB_AGG) | cnt[j]);
    }
    // global base of each digit: exclusive scan of this pass's digit histogram
    const uint32_t* gh = smeta + 4 + pass * RADIX;
    uint32_t g[4], s4 = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        g[j] = gh[4 * t + j];
        s4 += g[j];
    }
    uint32_t incl = wave_incl_add(s4);
    if (lane == 63) wsum[w] = incl;
    uint32_t excl[4] = {0u, 0u, 0u, 0u};
    int q[4];
    bool done[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        q[j] = (int)vid - 1;
        done[j] = vid == 0;
    }
    while (!(done[0] && done[1] && done[2] && done[3])) {
        uint32_t x[4][LB_WIN];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int m = 0; m < LB_WIN; ++m)
                x[j][m] = (!done[j] && q[j] - m >= 0) ? lb_load(&lb[(size_t)(q[j] - m) * RADIX + 4 * t + j]) : LB_PRE;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (done[j]) continue;
            int m = 0;
            for (; m < LB_WIN; ++m) {
                const uint32_t y = x[j][m];
                if (y == 0u) break;  // not published yet: poll it again
                excl[j] += y & LB_MASK;
                if (y & LB_PRE) {
                    done[j] = true;
                    break;
                }
            }
            q[j] -= m;
        }
    }
    if (vid != 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) lb_store(&lb[(size_t)vid * RADIX + 4 * t + j], LB_PRE | (excl[j] + cnt[j]));
    }
    __syncthreads();
    uint32_t gb = incl - s4;
    for (int q2 = 0; q2 < w; ++q2) gb += wsum[q2];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        running[4 * t + j] = gb + excl[j];
        gb += g[j];
    }
    __syncthreads();
    const unsigned long long lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    // (1) rank within the wave's contiguous chunk: running per-digit counts in wc[w][*] (only this
    //     wave touches its row, and one wave's LDS operations execute in order: no barrier)
    uint32_t lrank[ITEMS];
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const uint32_t i = base + w * (64 * ITEMS) + it * 64 + lane;
        const bool valid = i < n;
        const uint32_t d = (k[it] >> shift) & (RADIX - 1);
        unsigned long long peers = ballot(valid);
#pragma unroll
        for (int b = 0; b < RADIX_BITS; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long bb = ballot(bit);
            peers &= bit ? bb : ~bb;
        }
        const uint32_t before = valid ? wc[w * RADIX + d] : 0u;
        lrank[it] = before + __popcll(peers & lt);
        if (valid && (peers & lt) == 0ull) wc[w * RADIX + d] = before + __popcll(peers);
    }
    __syncthreads();
    // (2) per digit: wave bases = tile base of the digit + counts of the earlier waves
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t d = 4 * t + j;
        uint32_t acc = running[d];
#pragma unroll
        for (int q2 = 0; q2 < BLOCK / 64; ++q2) {
            const uint32_t c = wc[q2 * RADIX + d];
            wc[q2 * RADIX + d] = acc;
            acc += c;
        }
    }
    __syncthreads();
    // (3) scatter
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const uint32_t i = base + w * (64 * ITEMS) + it * 64 + lane;
        if (i < n) {
            const uint32_t off = wc[w * RADIX + ((k[it] >> shift) & (RADIX - 1))] + lrank[it];
            kout[off] = k[it];
            vout[off] = v[it];
        }
    }
}

constexpr uint32_t OS_BLOCK_N = 1024;  // k_onesweep_wide's workgroup

// Corner normals and (j.tri set) triangle records (v0, e1, e2, id) of every triangle — what k_gather writes
// with with_nrm / with_tri set — by `nblk` workgroups of OS_BLOCK_N lanes, grid-stride, each staged through `stage`
// (12 * OS_BLOCK_N floats) for whole-float4 stores. The build reads the records only once the keys are
// sorted (the chunk kernel) and the normals never (the trace shades with them), so on the
// top-digit-first path they are gathered by extra workgroups of that pass's launch: its few dozen to ~140
// tiles leave most CUs idle while their look-back chain runs, and the gather keeps only the boxes.
struct RecJob {
    const MeshDesc* meshes;
    uint32_t nm, n, nblk;
    float4* tri;
    float* nrm;
};
// The mesh table is copied into LDS after the staging area (up to RJ_LDS_MESHES meshes), so that each
// triangle's mesh search costs LDS round trips instead of dependent global ones.
constexpr uint32_t RJ_LDS_MESHES = 256;
__device__ void gather_records(const RecJob& j, uint32_t blk, float* stage) {
    float4* st4 = reinterpret_cast<float4*>(stage);
    MeshDesc* lm = reinterpret_cast<MeshDesc*>(stage + 12 * OS_BLOCK_N);
    const bool in_lds = j.nm <= RJ_LDS_MESHES;
    if (in_lds)
        for (uint32_t t = threadIdx.x; t < j.nm; t += OS_BLOCK_N) lm[t] = j.meshes[t];
    __syncthreads();
    const MeshDesc* mt = in_lds ? lm : j.meshes;
    for (uint32_t g0 = blk * OS_BLOCK_N; g0 < j.n; g0 += j.nblk * OS_BLOCK_N) {
        const uint32_t g = g0 + threadIdx.x, cnt = min(j.n - g0, OS_BLOCK_N);
        float nv[9];
        if (g < j.n) {
            uint32_t a = 0, b = j.nm;
            while (b - a > 1) {
                const uint32_t mid = (a + b) >> 1;
                if (mt[mid].tri_offset <= g) a = mid;
                else b = mid;
            }
            const MeshDesc md = mt[a];
            const uint32_t f = g - md.tri_offset;
            const uint32_t iv[3] = {md.idx[3 * f], md.idx[3 * f + 1], md.idx[3 * f + 2]};
            // k_gather's operations
            vec3f p0 = v3(0.0f, 0.0f, 0.0f), p1 = p0, p2 = p0;
            if (j.tri) {
                p0 = v3(md.pos[3 * iv[0]], md.pos[3 * iv[0] + 1], md.pos[3 * iv[0] + 2]);
                p1 = v3(md.pos[3 * iv[1]], md.pos[3 * iv[1] + 1], md.pos[3 * iv[1] + 2]);
                p2 = v3(md.pos[3 * iv[2]], md.pos[3 * iv[2] + 1], md.pos[3 * iv[2] + 2]);
            }
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c) nv[3 * k + c] = md.nrm[3 * iv[k] + c];
            if (j.tri) {
                const vec3f e1 = sub(p1, p0), e2 = sub(p2, p0);
                st4[3 * threadIdx.x + 0] = make_float4(p0.x, p0.y, p0.z, u2f(g));
                st4[3 * threadIdx.x + 1] = make_float4(e1.x, e1.y, e1.z, 0.0f);
                st4[3 * threadIdx.x + 2] = make_float4(e2.x, e2.y, e2.z, 0.0f);
            }
        }
        if (j.tri) {
            __syncthreads();
            for (uint32_t q = threadIdx.x; q < 3 * cnt; q += OS_BLOCK_N) j.tri[3 * (size_t)g0 + q] = st4[q];
            __syncthreads();
        }
        if (g < j.n)
#pragma unroll
            for (int k = 0; k < 9; ++k) stage[9 * threadIdx.x + k] = nv[k];
        __syncthreads();
        if (cnt == OS_BLOCK_N) {
            float4* nd = reinterpret_cast<float4*>(j.nrm + 9 * (size_t)g0);
            for (uint32_t q = threadIdx.x; q < 9 * OS_BLOCK_N / 4; q += OS_BLOCK_N) nd[q] = st4[q];
        } else {
            for (uint32_t q = threadIdx.x; q < 9 * cnt; q += OS_BLOCK_N) j.nrm[9 * (size_t)g0 + q] = stage[q];
        }
        __syncthreads();
    }
}

// A pass with 1024-thread workgroups: one digit per thread, so the look-back polls a window of
// OS_LB_WIN predecessor words per digit for the price of 4 x LB_WIN in a 256-lane tile (on_tile), and
// 16 waves rank a tile in parallel. On MI355X the look-back words live beyond the per-XCD L2s (agent scope), so one
// look-back step costs a fabric round trip: with every tile resident at once a tile walks back about
// tiles / (2 x window) steps, which a 32-word window keeps to a few.
constexpr int OS_WAVES = OS_BLOCK_N / 64;
constexpr int OS_BLOCK = OS_BLOCK_N;
constexpr int OS_LB_WIN = 32;
static_assert(OS_BLOCK == (int)RADIX, "one digit per thread");

// LDS of one wide one-sweep tile: k_onesweep_wide's own, or k_bucket_sort<1024>'s when it runs the LSD
// fallback (BsLds has the same arrays).
struct OwShared {
    uint32_t* wc;       // [OS_WAVES][RADIX]: per-wave digit counts, then the tile in digit order
    uint32_t* running;  // [RADIX]
    uint32_t* wsum;     // [OS_WAVES]
    uint32_t* lsum;     // [OS_WAVES]
};

// The ranking, look-back and scatter of one wide one-sweep tile whose keys and values are in registers
// (item it of wave w, lane l: tile position w * 64 * ITEMS + it * 64 + l); running[] and wc[] zeroed and
// a barrier passed by the caller; g = digit t's global count.
template <int ITEMS, bool C, class Diag, bool RANK = false>
__device__ __forceinline__ void ow_rank(const Diag& diag, const OwShared& S, const uint32_t (&k)[ITEMS],
                                        const uint32_t (&v)[ITEMS], uint32_t g, uint32_t* __restrict__ kout,
                                        uint32_t* __restrict__ vout, uint32_t n, int pass, int passes,
                                        uint32_t* __restrict__ smeta, uint32_t lbs, uint32_t vid,
                                        const uint16_t* srank = nullptr) {
    const int t = threadIdx.x, w = t >> 6, lane = t & 63;
    uint32_t* const wc = S.wc;
    uint32_t* const running = S.running;
    const uint32_t base = vid * (OS_BLOCK * ITEMS);
    const int shift = pass * RADIX_BITS;
    uint32_t* lb = smeta + 4 + (size_t)passes * RADIX + (size_t)pass * lbs * RADIX;
    int q = (int)vid - 1;
    bool done = vid == 0;
    uint32_t x[OS_LB_WIN];
    // (1) rank within the wave's contiguous chunk (running per-digit counts in wc[w][*]); the tile
    // histogram comes from the same ballots (one LDS atomic per digit run of a wave instead of one per
    // key: a tile's keys share few digits on the top pass of a coherent mesh)
    const unsigned long long lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    uint32_t lrank[ITEMS];
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const uint32_t i = base + w * (64 * ITEMS) + it * 64 + lane;
        const bool valid = i < n;
        const uint32_t d = sort_digit<RANK>(k[it], shift, srank);
        unsigned long long peers = ballot(valid);
#pragma unroll
        for (int b = 0; b < RADIX_BITS; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long bb = ballot(bit);
            peers &= bit ? bb : ~bb;
        }
        const uint32_t before = valid ? wc[w * RADIX + d] : 0u;
        lrank[it] = before + __popcll(peers & lt);
        if (valid && (peers & lt) == 0ull) {
            wc[w * RADIX + d] = before + __popcll(peers);
            atomicAdd(&running[d], (uint32_t)__popcll(peers));
        }
    }
    __syncthreads();
    diag.mark(0);
    const uint32_t cnt = running[t];
    lb_store(&lb[(size_t)vid * RADIX + t], (vid == 0 ? LB_PRE : LB_AGG) | cnt);
    // the first look-back window is in flight during the scans below
#pragma unroll
    for (int m = 0; m < OS_LB_WIN; ++m)
        x[m] = (!done && q - m >= 0) ? lb_load(&lb[(size_t)(q - m) * RADIX + t]) : LB_PRE;
    diag.mark(1);
    // inclusive scans over the digits: global histogram (digit bases in the output) and this tile's
    // counts (digit starts inside the tile)
    const uint32_t incl = wave_incl_add(g), lincl = wave_incl_add(cnt);
    if (lane == 63) {
        S.wsum[w] = incl;
        S.lsum[w] = lincl;
    }
    uint32_t excl = 0;
    while (!done) {
        int m = 0;
        for (; m < OS_LB_WIN; ++m) {
            const uint32_t y = x[m];
            if (y == 0u) break;  // not published yet: poll it again
            excl += y & LB_MASK;
            if (y & LB_PRE) {
                done = true;
                break;
            }
        }
        q -= m;
        if (!done) {
#pragma unroll
            for (int m2 = 0; m2 < OS_LB_WIN; ++m2)
                x[m2] = q - m2 >= 0 ? lb_load(&lb[(size_t)(q - m2) * RADIX + t]) : LB_PRE;
        }
    }
    if (vid != 0) lb_store(&lb[(size_t)vid * RADIX + t], LB_PRE | (excl + cnt));
    diag.mark(2);
    __syncthreads();
    uint32_t gb = incl - g, ls = lincl - cnt;
    for (int q2 = 0; q2 < w; ++q2) {
        gb += S.wsum[q2];
        ls += S.lsum[q2];
    }
    // (2) digit t: tile-local wave bases; output slot of the tile's j-th key (digit order) = running[d] + j
    {
        uint32_t acc = ls;
#pragma unroll
        for (int q2 = 0; q2 < OS_WAVES; ++q2) {
            const uint32_t c = wc[q2 * RADIX + t];
            wc[q2 * RADIX + t] = acc;
            acc += c;
        }
    }
    running[t] = gb + excl - ls;
    __syncthreads();
    uint32_t lp[ITEMS];
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) lp[it] = wc[w * RADIX + sort_digit<RANK>(k[it], shift, srank)] + lrank[it];
    __syncthreads();
    // (3) the tile in digit order through LDS (over wc), then runs of consecutive output slots
    uint32_t* s_k = wc;
    uint32_t* s_v = s_k + OS_BLOCK * ITEMS;
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        if (base + w * (64 * ITEMS) + it * 64 + lane < n) {
            s_k[lp[it]] = k[it];
            s_v[lp[it]] = v[it];
        }
    }
    __syncthreads();
    diag.mark(3);
    const uint32_t tn = min(n - base, (uint32_t)(OS_BLOCK * ITEMS));
#pragma unroll
    for (int m = 0; m < ITEMS; ++m) {
        const uint32_t j = m * OS_BLOCK + t;
        if (j < tn) {
            const uint32_t key = s_k[j];
            const uint32_t off = running[sort_digit<RANK>(key, shift, srank)] + j;
            cst<C>(kout + off, key);
            cst<C>(vout + off, s_v[j]);
        }
    }
}

// One tile (ticket vid) of a one-sweep pass with OS_BLOCK lanes (one digit per thread). lbs: tiles per
// pass in the look-back area (its stride). wait_ctr: wait for that many (wait_for) tiles of the
// previous pass first (the LSD fallback's second pass in the same launch).
template <int ITEMS, bool C = false, class Diag, bool RANK = false>
__device__ __forceinline__ void ow_tile(const Diag& diag, const OwShared& S, const uint32_t* __restrict__ kin,
                                        const uint32_t* __restrict__ vin, uint32_t* __restrict__ kout,
                                        uint32_t* __restrict__ vout, uint32_t n, int pass, int passes,
                                        uint32_t* __restrict__ smeta, uint32_t lbs, uint32_t vid,
                                        const uint32_t* wait_ctr = nullptr, uint32_t wait_for = 0,
                                        const uint16_t* srank = nullptr) {
    static_assert(2 * OS_BLOCK * ITEMS <= OS_WAVES * RADIX, "the digit-ordered tile reuses wc");
    const int t = threadIdx.x, w = t >> 6, lane = t & 63;
    uint32_t* const wc = S.wc;
    uint32_t* const running = S.running;
    const uint32_t g = cld<C>(smeta + 4 + pass * RADIX + t);  // digit t's global count
    running[t] = 0;
#pragma unroll
    for (int q = 0; q < OS_WAVES; ++q) wc[q * RADIX + t] = 0;
    if (wait_ctr) coh_wait(wait_ctr, wait_for);
    const uint32_t base = vid * (OS_BLOCK * ITEMS);
    // one digit holds every key: the stable pass is the identity, so every tile copies itself (no
    // ranking, no look-back; all tiles read the same histogram and take this branch together)
    if (__syncthreads_or(g == n)) {
#pragma unroll
        for (int it = 0; it < ITEMS; ++it) {
            const uint32_t i = base + it * OS_BLOCK + t;
            if (i < n) {
                cst<C>(kout + i, cld<C>(kin + i));
                cst<C>(vout + i, cld<C>(vin + i));
            }
        }
        return;
    }
    uint32_t k[ITEMS], v[ITEMS];
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {  // each wave: a contiguous chunk of the tile (stability)
        const uint32_t i = min(base + w * (64 * ITEMS) + it * 64 + lane, n - 1);
        k[it] = cld<C>(kin + i);
        v[it] = cld<C>(vin + i);
    }
    ow_rank<ITEMS, C, Diag, RANK>(diag, S, k, v, g, kout, vout, n, pass, passes, smeta, lbs, vid, srank);
}


// The bucket plan of a top-digit-first sort, by one extra workgroup (OS_BLOCK lanes, lane t = digit t)
// of the top-digit pass's launch, beside its tiles: plan[PLAN_ORDER + i] = the i-th bucket with more
// than one key in (size class of 64 keys descending, digit) order, ~0u past them — workgroup b of
// k_bucket_sort sorts bucket b of that order, so the nonempty buckets dispatch first and the biggest in
// the first round (in digit order the 1,024-lane workgroups of empty and big buckets queued behind each
// other); plan[PLAN_START + d] = the first position of bucket d; plan[PLAN_FLAG] = some bucket holds
// skew_cap keys or more (the LSD fallback). Each bucket workgroup used to derive all of it from the
// histogram itself (~4 us of its ~9).
// C: the histogram was summed by this launch (device-coherent loads).
template <bool C = false>
__device__ void bucket_plan(const uint32_t* __restrict__ gh, uint32_t* __restrict__ plan, uint32_t skew_cap,
                            uint32_t* lds) {
    constexpr uint32_t NCLS = 128;
    const uint32_t t = threadIdx.x, w = t >> 6, lane = t & 63;
    uint32_t* cnt = lds;                    // [OS_WAVES][NCLS] per-wave class counts, then wave bases
    uint32_t* cbase = lds + OS_WAVES * NCLS;  // [NCLS] class bases
    uint32_t* wsum = cbase + NCLS;          // [OS_WAVES]
    const uint32_t c = cld<C>(gh + t);
    for (uint32_t i = t; i < OS_WAVES * NCLS; i += OS_BLOCK) cnt[i] = 0;
    // bucket starts: exclusive scan of the histogram over the digits
    uint32_t incl = wave_incl_add(c);
    if (lane == 63) wsum[w] = incl;
    const uint32_t cls = c <= 1 ? NCLS - 1 : NCLS - 2 - min(c >> 6, NCLS - 2);  // 0: the largest
    const unsigned long long lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    unsigned long long peers = ~0ull;
#pragma unroll
    for (int b = 0; b < 7; ++b) {
        const bool bit = (cls >> b) & 1u;
        const unsigned long long bb = ballot(bit);
        peers &= bit ? bb : ~bb;
    }
    __syncthreads();  // cnt zeroed, wsum in
    uint32_t start = incl - c;
    for (uint32_t q = 0; q < w; ++q) start += wsum[q];
    plan[PLAN_START + t] = start;
    if ((peers & lt) == 0ull) cnt[w * NCLS + cls] = (uint32_t)__popcll(peers);
    __syncthreads();
    if (t < NCLS) {  // class t: its waves' bases, then the classes' exclusive scan (two waves)
        uint32_t tot = 0;
#pragma unroll
        for (int q = 0; q < OS_WAVES; ++q) {
            const uint32_t x = cnt[q * NCLS + t];
            cnt[q * NCLS + t] = tot;
            tot += x;
        }
        uint32_t ci = wave_incl_add(tot);
        cbase[t] = ci - tot;
        if (lane == 63) wsum[w] = ci;  // waves 0, 1
    }
    __syncthreads();
    const uint32_t pos = cbase[cls] + (cls >= 64 ? wsum[0] : 0u) + cnt[w * NCLS + cls] + (uint32_t)__popcll(peers & lt);
    plan[PLAN_ORDER + pos] = c > 1 ? t : ~0u;  // the single-key and empty buckets are class NCLS - 1: last
    const bool big = __syncthreads_or(c >= skew_cap);
    if (t == 0) plan[PLAN_FLAG] = big ? 1u : 0u;
}

// One pass of the sort per launch: workgroups [0, nb) take tiles by ticket, the ones past them
// gather records and normals (rj.nblk, launch_onesweep). skew_cap > 0 (the top-digit pass of a
// top-digit-first sort, launched with 2 nb tile workgroups): when k_morton's top-digit histogram has a
// bucket of skew_cap keys or more — more than k_bucket_sort's cap = skew_cap - 1 — every workgroup sees it
// and the launch runs the LSD passes 0 and 1 instead (tickets [0, nb) pass 0 keys2 -> keys, [nb, 2 nb)
// pass 1 keys -> keys2 once every pass-0 tile is done; k_bucket_sort then runs pass 2). The tile
// counter of pass 0 (the skew word) is left nonzero, which tells the host the build took that path.
template <int ITEMS, bool RANK = false>
__global__ __launch_bounds__(OS_BLOCK) void k_onesweep_wide(const uint32_t* __restrict__ kin,
                                                            const uint32_t* __restrict__ vin,
                                                            uint32_t* __restrict__ kout, uint32_t* __restrict__ vout,
                                                            uint32_t n, int pass, int passes,
                                                            uint32_t* __restrict__ smeta, uint32_t nb, uint32_t lbs,
                                                            RecJob rj, uint32_t skew_cap, uint32_t* __restrict__ plan,
                                                            const uint32_t* __restrict__ topmap = nullptr) {
    __shared__ uint32_t s_vid;
    __shared__ uint32_t wsum[OS_WAVES], lsum[OS_WAVES];
    __shared__ uint32_t running[RADIX];
    __shared__ uint32_t wc[OS_WAVES][RADIX];  // per-wave digit counts, then the tile in digit order
    static_assert(12 * OS_BLOCK + RJ_LDS_MESHES * sizeof(MeshDesc) / 4 <= OS_WAVES * RADIX,
                  "the records' staging and mesh table reuse wc");
    const uint32_t tile_wgs = skew_cap ? 2 * nb : nb;
    if (blockIdx.x >= tile_wgs) {  // workgroups past the tiles: triangle records and normals, then the plan
        if (blockIdx.x - tile_wgs < rj.nblk) gather_records(rj, blockIdx.x - tile_wgs, reinterpret_cast<float*>(&wc[0][0]));
        else bucket_plan(smeta + 4 + pass * RADIX, plan, skew_cap, &wc[0][0]);
        return;
    }
    const int t = threadIdx.x;
    const bool skew = skew_cap && __syncthreads_or(smeta[4 + pass * RADIX + t] >= skew_cap);
    if (!skew && blockIdx.x >= nb) return;
    BDIAG(2 + pass);
    if (t == 0) s_vid = atomicAdd(&smeta[skew ? 0 : pass], 1u);
    __syncthreads();
    const uint32_t vid = s_vid;
    const OwShared S{&wc[0][0], running, wsum, lsum};
    if constexpr (RANK) {  // the ranked top digit (build_top_rank): a reference-mode pair sort's last pass
        __shared__ uint16_t srank[TOP_VALUES];
        __shared__ uint32_t swpre[64];
        build_top_rank(topmap, srank, swpre, OS_BLOCK);
        __syncthreads();
        ow_tile<ITEMS, false, decltype(BDIAG_OBJ), true>(BDIAG_OBJ, S, kin, vin, kout, vout, n, pass, passes, smeta,
                                                         lbs, vid, nullptr, 0, srank);
        return;
    }
    if (!skew) {
        ow_tile<ITEMS>(BDIAG_OBJ, S, kin, vin, kout, vout, n, pass, passes, smeta, lbs, vid);
    } else if (vid < nb) {  // LSD pass 0: Morton output (kin) -> kout
        ow_tile<ITEMS, true>(BDIAG_OBJ, S, kin, vin, kout, vout, n, 0, passes, smeta, lbs, vid);
        coh_done(smeta + 3);
    } else {  // LSD pass 1: kout -> kin, after every pass-0 tile
        ow_tile<ITEMS, true>(BDIAG_OBJ, S, kout, vout, const_cast<uint32_t*>(kin), const_cast<uint32_t*>(vin), n, 1,
                             passes, smeta, lbs, vid - nb, smeta + 3, nb);
    }
}


// ---- small sorts: most significant digit first, then each bucket on its own -------------------------
// For MSD_MIN_N <= n <= MSD_MAX_N (msd_sort) the build sorts by the top digit first (one k_onesweep_wide pass, stable) and
// then sorts each of the RADIX buckets by the two lower digits in one workgroup (k_bucket_sort), in
// place: the same stable order as three LSD passes — (top digit, lower digits, index) — in two launches
// instead of three. A bucket of at most BS_CAP keys is sorted in LDS (two 10-bit passes, ranked by
// ballots in index order as in k_onesweep_wide). When k_morton's top-digit histogram holds a larger
// bucket (a skewed scene: a far triangle stretches the scene box, and most keys share their top digit),
// the same two launches run the three LSD passes instead, decided on the device from that histogram:
// k_onesweep_wide passes 0 and 1 (the second after the first's tiles, by ticket), k_bucket_sort pass 2.
constexpr uint32_t MSD_MAX_N = 1u << 22;   // bunny 0.080 -> 0.067 ms, armadillo 0.122 -> 0.100
constexpr uint32_t MSD_WIDE_N = 1u << 19;  // above: 1024-lane bucket workgroups (8,192 keys in LDS, one workgroup per CU)
constexpr uint32_t MSD_MIN_N = 1u << 14;   // below: a few one-sweep tiles per pass are cheaper than 1024 bucket workgroups
constexpr int BS_ITEMS = 8;  // keys per lane at most: a bucket of up to BS_BLOCK * 8 keys sorts in LDS
__device__ __forceinline__ uint32_t blocks_for_dev(uint32_t n, uint32_t per) { return (n + per - 1) / per; }

template <int BS_BLOCK>
struct BsLds {
    static constexpr int BS_WAVES = BS_BLOCK / 64;
    static constexpr uint32_t BS_CAP = BS_BLOCK * BS_ITEMS;
    uint32_t wc[BS_WAVES][RADIX];  // per-wave digit counts, then output bases
    uint32_t k[BS_CAP], v[BS_CAP];
    uint32_t run[RADIX];           // LSD fallback: the one-sweep tile's running digit bases
    uint32_t wsum[BS_WAVES];
    uint32_t red[BS_WAVES];
};

// Ranks the tile's keys (wave w: items [w * 64 * ITEMS, +64 * ITEMS), lane order within an item row)
// by digit (key >> shift) & (RADIX - 1), stably: lrank = rank among equal digits of the same wave, wc[w][d]
// = the wave's count of digit d.
template <int BS_BLOCK>
__device__ __forceinline__ void bs_rank(BsLds<BS_BLOCK>& L, const uint32_t (&k)[BS_ITEMS], uint32_t (&lrank)[BS_ITEMS], int shift,
                                        uint32_t tn, int ie) {
    constexpr int BS_WAVES = BS_BLOCK / 64;
    const int t = threadIdx.x, w = t >> 6, lane = t & 63;
    for (int d = t; d < BS_WAVES * (int)RADIX; d += BS_BLOCK) (&L.wc[0][0])[d] = 0;
    __syncthreads();
    const unsigned long long lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
#pragma unroll
    for (int it = 0; it < BS_ITEMS; ++it) {
        if (it >= ie) break;
        const uint32_t i = w * (64 * ie) + it * 64 + lane;
        const bool valid = i < tn;
        const uint32_t d = (k[it] >> shift) & (RADIX - 1);
        unsigned long long peers = ballot(valid);
#pragma unroll
        for (int b = 0; b < RADIX_BITS; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long bb = ballot(bit);
            peers &= bit ? bb : ~bb;
        }
        const uint32_t before = valid ? L.wc[w][d] : 0u;
        lrank[it] = before + __popcll(peers & lt);
        if (valid && (peers & lt) == 0ull) L.wc[w][d] = before + __popcll(peers);
    }
    __syncthreads();
}

// Per-wave output bases wc[w][d] = base(d) + (digit d's keys in the waves before w). LDS path (run ==
// nullptr): base(d) = exclusive scan over the digits of the tile's totals. Global path: base(d) = run[d],
// the running base of digit d over the tiles before, which then advances by the tile's count of d.
template <int BS_BLOCK>
__device__ __forceinline__ void bs_bases(BsLds<BS_BLOCK>& L, uint32_t* run) {
    constexpr int BS_WAVES = BS_BLOCK / 64;
    const int t = threadIdx.x, w = t >> 6, lane = t & 63;
    constexpr int DPT = RADIX / BS_BLOCK;  // digits per thread (4)
    uint32_t tot[DPT], sum = 0;
#pragma unroll
    for (int j = 0; j < DPT; ++j) {
        const int d = t * DPT + j;
        uint32_t c = 0;
#pragma unroll
        for (int q = 0; q < BS_WAVES; ++q) c += L.wc[q][d];
        tot[j] = c;
        sum += c;
    }
    uint32_t incl = wave_incl_add(sum);
    if (lane == 63) L.wsum[w] = incl;
    __syncthreads();
    uint32_t excl = incl - sum;
    for (int q = 0; q < w; ++q) excl += L.wsum[q];
#pragma unroll
    for (int j = 0; j < DPT; ++j) {
        const int d = t * DPT + j;
        uint32_t acc = run ? run[d] : excl;
#pragma unroll
        for (int q = 0; q < BS_WAVES; ++q) {
            const uint32_t c = L.wc[q][d];
            L.wc[q][d] = acc;
            acc += c;
        }
        if (run) run[d] = acc;
        excl += tot[j];
    }
    __syncthreads();
}

// The bucket of each workgroup, its start and the skew flag come from the plan the top-digit pass's launch
// wrote (bucket_plan). Also the LSD fallback's last pass: when a top-digit bucket holds more than the LDS
// cap (the flag; k_onesweep_wide
// ran the LSD passes 0 and 1 instead of the top-digit pass, into keys2/vals2), the workgroups run the
// one-sweep pass 2 over keys2 -> keys in tiles of the top-digit pass's size (wide_items keys per lane
// of a 1,024-lane tile; 256-lane workgroups take the same tiles at 4 wide_items per lane, or half of
// one at 8 keys per lane for one-key-per-lane tiles), and no bucket is sorted.
template <int BS_BLOCK>
__global__ __launch_bounds__(BS_BLOCK) void k_bucket_sort(uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                          uint32_t* __restrict__ keys2, uint32_t* __restrict__ vals2,
                                                          uint32_t* __restrict__ meta, const uint32_t* __restrict__ plan,
                                                          uint32_t n, uint32_t nb, int wide_items) {
    BDIAG(3);
    __shared__ BsLds<BS_BLOCK> L;
    const int t = threadIdx.x, w = t >> 6, lane = t & 63;
    const uint32_t* gh = meta + META_GHIST + 2 * RADIX;  // top-digit histogram (k_morton)
    // the plan's skew flag: the test k_onesweep_wide made on the same histogram
    if (plan[PLAN_FLAG]) {
        uint32_t* smeta = meta + META_COUNTERS;
        __shared__ uint32_t s_vid;
        const int items = BS_BLOCK == 1024 ? 8 : wide_items == 1 ? 8 : 16;
        if (blockIdx.x >= blocks_for_dev(n, BS_BLOCK * items)) return;
        if (t == 0) s_vid = atomicAdd(&smeta[2], 1u);
        __syncthreads();
        if constexpr (BS_BLOCK == 1024) {
            const OwShared S{&L.wc[0][0], L.run, L.wsum, L.red};
            ow_tile<8>(NoDiag(), S, keys2, vals2, keys, vals, n, 2, RADIX_PASSES, smeta, nb, s_vid);
        } else if (items == 8) {
            on_tile<8>(&L.wc[0][0], L.run, L.wsum, keys2, vals2, keys, vals, n, 2, RADIX_PASSES, smeta, nb, s_vid);
        } else {
            on_tile<16>(&L.wc[0][0], L.run, L.wsum, keys2, vals2, keys, vals, n, 2, RADIX_PASSES, smeta, nb, s_vid);
        }
        return;
    }
    // workgroup b sorts the plan's b-th bucket: the nonempty ones largest first (bucket_plan)
    const uint32_t d = plan[PLAN_ORDER + blockIdx.x];
    if (d == ~0u) return;
    const uint32_t c = gh[d], start = plan[PLAN_START + d];
    uint32_t k[BS_ITEMS], v[BS_ITEMS], lrank[BS_ITEMS];
    // the bucket in LDS (c <= cap <= BS_CAP: larger buckets took the LSD fallback above): two passes,
    // one load, one store. Items per lane sized to the bucket, so that all waves share the ranking chains
    const int ie = (int)((c + BS_BLOCK - 1) / BS_BLOCK);
#pragma unroll
    for (int it = 0; it < BS_ITEMS; ++it) {
        if (it >= ie) break;
        const uint32_t i = w * (64 * ie) + it * 64 + lane;
        k[it] = i < c ? keys[start + i] : 0u;
        v[it] = i < c ? vals[start + i] : 0u;
    }
    for (int pass = 0; pass < 2; ++pass) {
        const int shift = pass * RADIX_BITS;
        BDIAG_MARK(2 * pass);
        bs_rank(L, k, lrank, shift, c, ie);
        BDIAG_MARK(2 * pass + 1);
        bs_bases(L, nullptr);
#pragma unroll
        for (int it = 0; it < BS_ITEMS; ++it) {
            if (it >= ie) break;
            const uint32_t i = w * (64 * ie) + it * 64 + lane;
            if (i < c) {
                const uint32_t o = L.wc[w][(k[it] >> shift) & (RADIX - 1)] + lrank[it];
                L.k[o] = k[it];
                L.v[o] = v[it];
            }
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < BS_ITEMS; ++it) {
            if (it >= ie) break;
            const uint32_t i = w * (64 * ie) + it * 64 + lane;
            k[it] = i < c ? L.k[i] : 0u;
            v[it] = i < c ? L.v[i] : 0u;
        }
        __syncthreads();
    }
#pragma unroll
    for (int it = 0; it < BS_ITEMS; ++it) {
        if (it >= ie) break;
        const uint32_t i = w * (64 * ie) + it * 64 + lane;
        if (i < c) {
            keys[start + i] = k[it];
            vals[start + i] = v[it];
        }
    }
}

// One-sweep tile: small sorts are latency-bound (a few dozen tiles, each a serial chain of load,
// look-back, rank, scatter), so they take short tiles; big ones take long tiles, which halve the
// look-back work per key. Measured on MI355X (tools/build_bench.py).
constexpr uint32_t OSW_TINY_N = 1u << 17;   // up to this many keys: 1024-key tiles (1 per thread; bunny build 0.114 -> 0.110 ms)
constexpr uint32_t OSW_SMALL_N = 1u << 17;  // up to this many keys (above OSW_TINY_N): 2048-key tiles (2 per thread)
constexpr uint32_t OSW_MID_N = 1u << 19;    // up to this many keys: 4096-key tiles; above, 8192
inline int onesweep_items(uint32_t n) {
    return n <= OSW_TINY_N ? 1 : n <= OSW_SMALL_N ? 2 : n <= OSW_MID_N ? 4 : 8;
}
inline uint32_t onesweep_tiles(uint32_t n) { return n ? blocks_for(n, OS_BLOCK * onesweep_items(n)) : 1u; }

// One pass (k_onesweep_wide) over n keys, the tile size by onesweep_items.
// rj.nblk > 0: that many more workgroups gather the triangle records and corner normals (gather_records).
// skew_cap > 0: the top-digit pass of a top-digit-first sort, with the LSD fallback's second set of tiles
// and one more workgroup for the bucket plan (written to `plan`).
// topmap: the ranked top digit (no records job, no skew fallback on that path).
template <bool RANK>
void launch_onesweep_as(uint32_t grid, const uint32_t* ki, const uint32_t* vi, uint32_t* ko, uint32_t* vo, uint32_t n,
                        int pass, int passes, uint32_t* smeta, hipStream_t s, uint32_t nb, RecJob rj, uint32_t skew_cap,
                        uint32_t* plan, const uint32_t* topmap) {
    switch (onesweep_items(n)) {
        case 1: k_onesweep_wide<1, RANK><<<grid, OS_BLOCK, 0, s>>>(ki, vi, ko, vo, n, pass, passes, smeta, nb, nb, rj, skew_cap, plan, topmap); break;
        case 2: k_onesweep_wide<2, RANK><<<grid, OS_BLOCK, 0, s>>>(ki, vi, ko, vo, n, pass, passes, smeta, nb, nb, rj, skew_cap, plan, topmap); break;
        case 4: k_onesweep_wide<4, RANK><<<grid, OS_BLOCK, 0, s>>>(ki, vi, ko, vo, n, pass, passes, smeta, nb, nb, rj, skew_cap, plan, topmap); break;
        default: k_onesweep_wide<8, RANK><<<grid, OS_BLOCK, 0, s>>>(ki, vi, ko, vo, n, pass, passes, smeta, nb, nb, rj, skew_cap, plan, topmap); break;
    }
}
void launch_onesweep(const uint32_t* ki, const uint32_t* vi, uint32_t* ko, uint32_t* vo, uint32_t n, int pass,
                     int passes, uint32_t* smeta, hipStream_t s, RecJob rj = RecJob{}, uint32_t skew_cap = 0,
                     uint32_t* plan = nullptr, const uint32_t* topmap = nullptr) {
    const uint32_t nb = onesweep_tiles(n);
    if (topmap)
        launch_onesweep_as<true>(nb, ki, vi, ko, vo, n, pass, passes, smeta, s, nb, rj, 0, nullptr, topmap);
    else
        launch_onesweep_as<false>((skew_cap ? 2 * nb + 1 : nb) + rj.nblk, ki, vi, ko, vo, n, pass, passes, smeta, s,
                                  nb, rj, skew_cap, plan, nullptr);
}
