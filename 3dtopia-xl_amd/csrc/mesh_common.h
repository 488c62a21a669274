// What every stage of the mesh export path (mcubes.hip, texbake.hip, meshclean.hip, meshdecim.hip, meshfield.hip,
// material.hip) shares, stated once.  Include inside the translation unit's anonymous namespace, after common.h.
//
// Block-prefix compaction: a kernel counts its items per block of PTS (block_sums), scan_kernel - ONE workgroup - turns
// the block sums into exclusive offsets plus totals, and a second kernel walks the same blocks in the same order and
// places each item at offset + block_prefix.  Every block covers PTS consecutive items, thread t the items
// base + r * THREADS + t (r = 0 .. ROUNDS - 1), so the order inside a block is (r, t) and the per-round prefix keeps it.
// sum_kernel / place_kernel are that pair for an int array (flags -> ranks, ints -> offsets); a stage whose predicate is
// not an array keeps its own fused pair and calls scan_blocks between them.
#pragma once

constexpr int THREADS = 256;
constexpr int ROUNDS = 4;
constexpr int PTS = THREADS * ROUNDS;   // items per block of the block-prefix kernels
constexpr int SCAN_THREADS = 1024;

// ------------------------------------------------------------------ device side

__device__ __forceinline__ int lanes_below(unsigned long long m) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

__device__ __forceinline__ int wave_min(int x) {
    for (int o = 32; o > 0; o >>= 1) x = min(x, __shfl_xor(x, o));
    return x;
}
__device__ __forceinline__ int wave_max(int x) {
    for (int o = 32; o > 0; o >>= 1) x = max(x, __shfl_xor(x, o));
    return x;
}
__device__ __forceinline__ int wave_sum(int x) {
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

// The waves' sums in s_wave -> (sum of the waves in front of this one, the block's sum).  Every thread of the block calls it.
__device__ __forceinline__ int waves_before(int* s_wave, int& total) {
    const int wave = threadIdx.x >> 6;
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) {
        off += (w < wave) ? s_wave[w] : 0;
        tot += s_wave[w];
    }
    __syncthreads();
    total = tot;
    return off;
}

// Exclusive prefix of a 0 / 1 flag over the block's 256 threads in thread order; `total` = the block's sum.  Every
// thread of the block calls it.
__device__ __forceinline__ int block_prefix(bool c, int* s_wave, int& total) {
    const unsigned long long b = __ballot(c);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = __popcll(b);
    return waves_before(s_wave, total) + lanes_below(b);
}

// The same of a count c in 0 .. 7, one ballot per bit.
__device__ __forceinline__ int block_prefix3(int c, int* s_wave, int& total) {
    const unsigned long long b0 = __ballot(c & 1), b1 = __ballot(c & 2), b2 = __ballot(c & 4);
    const int pre = lanes_below(b0) + 2 * lanes_below(b1) + 4 * lanes_below(b2);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = __popcll(b0) + 2 * __popcll(b1) + 4 * __popcll(b2);
    return waves_before(s_wave, total) + pre;
}

// The same of any int.
__device__ __forceinline__ int block_excl(int x, int* s_wave, int& total) {
    const int lane = threadIdx.x & 63;
    int inc = x;
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(inc, o);
        if (lane >= o) inc += y;
    }
    if (lane == 63) s_wave[threadIdx.x >> 6] = inc;
    return waves_before(s_wave, total) + inc - x;
}

// Block sums of up to two counters: thread 0 writes (a, b) of block blockIdx.x to bsum[2 * blockIdx.x + {0, 1}].
__device__ __forceinline__ void block_sums(int a, int b, long long* bsum) {
    __shared__ int s_red[2][THREADS / 64];
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_down(a, o);
        b += __shfl_down(b, o);
    }
    if ((threadIdx.x & 63) == 0) { s_red[0][threadIdx.x >> 6] = a; s_red[1][threadIdx.x >> 6] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        long long x = 0, y = 0;
        for (int w = 0; w < THREADS / 64; ++w) { x += s_red[0][w]; y += s_red[1][w]; }
        bsum[2 * (size_t)blockIdx.x] = x;
        bsum[2 * (size_t)blockIdx.x + 1] = y;
    }
}

// One workgroup: exclusive block offsets of both counters in place, totals [2] = the sums.  Thread t owns the contiguous
// run [t * per, (t + 1) * per) of the block sums.
__global__ __launch_bounds__(SCAN_THREADS) void scan_kernel(long long* __restrict__ bsum, int nblk,
                                                            long long* __restrict__ totals) {
    __shared__ long long s[2][SCAN_THREADS];
    const int per = (nblk + SCAN_THREADS - 1) / SCAN_THREADS;
    const int lo = min(nblk, (int)threadIdx.x * per), hi = min(nblk, lo + per);
    long long a = 0, b = 0;
    for (int q = lo; q < hi; ++q) { a += bsum[2 * (size_t)q]; b += bsum[2 * (size_t)q + 1]; }
    s[0][threadIdx.x] = a;
    s[1][threadIdx.x] = b;
    __syncthreads();
    for (int o = 1; o < SCAN_THREADS; o <<= 1) {   // inclusive Hillis-Steele scan
        const long long xa = threadIdx.x >= o ? s[0][threadIdx.x - o] : 0, xb = threadIdx.x >= o ? s[1][threadIdx.x - o] : 0;
        __syncthreads();
        s[0][threadIdx.x] += xa;
        s[1][threadIdx.x] += xb;
        __syncthreads();
    }
    a = s[0][threadIdx.x] - a;
    b = s[1][threadIdx.x] - b;
    for (int q = lo; q < hi; ++q) {
        const long long va = bsum[2 * (size_t)q], vb = bsum[2 * (size_t)q + 1];
        bsum[2 * (size_t)q] = a;
        bsum[2 * (size_t)q + 1] = b;
        a += va;
        b += vb;
    }
    if (threadIdx.x == SCAN_THREADS - 1) { totals[0] = s[0][threadIdx.x]; totals[1] = s[1][threadIdx.x]; }
}

__global__ __launch_bounds__(THREADS) void fill_kernel(int* __restrict__ a, int n, int value) {
    const int t = blockIdx.x * THREADS + threadIdx.x;
    if (t < n) a[t] = value;
}

__global__ __launch_bounds__(THREADS) void sum_kernel(const int* __restrict__ x, int n, int as_flag,
                                                      long long* __restrict__ bsum) {
    int c = 0;
    for (int r = 0; r < ROUNDS; ++r) {
        const int t = blockIdx.x * PTS + r * THREADS + threadIdx.x;
        if (t < n) c += as_flag ? (x[t] != 0 ? 1 : 0) : x[t];
    }
    block_sums(c, 0, bsum);
}

// as_flag: out[t] = position of t among the set flags (-1 when clear); else out[t] = exclusive prefix sum, and out2[t]
// too where out2 is given
__global__ __launch_bounds__(THREADS) void place_kernel(const int* __restrict__ x, int n, int as_flag,
                                                        const long long* __restrict__ boff, int* __restrict__ out,
                                                        int* __restrict__ out2) {
    __shared__ int s_wave[THREADS / 64];
    long long run = boff[2 * (size_t)blockIdx.x];
    for (int r = 0; r < ROUNDS; ++r) {
        const int t = blockIdx.x * PTS + r * THREADS + threadIdx.x;
        const int val = t < n ? x[t] : 0;
        int tot;
        if (as_flag) {
            const int pre = block_prefix(val != 0, s_wave, tot);
            if (t < n) out[t] = val != 0 ? (int)(run + pre) : -1;
        } else {
            const int pre = block_excl(val, s_wave, tot);
            if (t < n) {
                out[t] = (int)(run + pre);
                if (out2) out2[t] = (int)(run + pre);
            }
        }
        run += tot;
    }
}

// ------------------------------------------------------------------ host side

constexpr size_t ALIGN = 256;
constexpr int64_t I31 = (int64_t)1 << 31;

inline size_t align_up(size_t v) { return (v + ALIGN - 1) / ALIGN * ALIGN; }
inline int nblocks(int64_t n, int per) { return (int)((n + per - 1) / per); }

// A workspace layout: take() hands out ALIGN-aligned offsets in sequence, `total` ends as the workspace's size.
struct Arena {
    size_t total = 0;
    size_t take(size_t bytes) {
        const size_t o = total;
        total += align_up(bytes);
        return o;
    }
};

#define PRIMX_TRY(x)                   \
    do {                               \
        if (int s__ = (x)) return s__; \
    } while (0)

inline int zero(void* p, size_t bytes, hipStream_t st, const char* name) {
    if (hipMemsetAsync(p, 0, bytes, st) != hipSuccess) {
        primx_set_error("%s: hipMemsetAsync failed", name);
        return PRIMX_ELAUNCH;
    }
    return PRIMX_OK;
}

inline int fill(int* a, int64_t n, int value, hipStream_t st, const char* name) {
    if (n <= 0) return PRIMX_OK;
    hipLaunchKernelGGL(fill_kernel, dim3(nblocks(n, THREADS)), dim3(THREADS), 0, st, a, (int)n, value);
    PRIMX_CHECK_LAUNCH(name);
    return PRIMX_OK;
}

// the block sums of nblk blocks -> exclusive block offsets in place, the two totals in tot
inline int scan_blocks(long long* bsum, int nblk, long long* tot, hipStream_t st, const char* name) {
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, bsum, nblk, tot);
    PRIMX_CHECK_LAUNCH(name);
    return PRIMX_OK;
}

// flags x [n] -> out [n] (position among the set flags, -1 when clear), or ints -> exclusive offsets (in out2 as well
// where it is given); the total in tot[0].  bsum: block sums of n items.
inline int scan(const int* x, int n, bool as_flag, int* out, int* out2, long long* bsum, long long* tot, hipStream_t st,
                const char* name) {
    if (n == 0) return zero(tot, 16, st, name);
    const int nblk = nblocks(n, PTS);
    hipLaunchKernelGGL(sum_kernel, dim3(nblk), dim3(THREADS), 0, st, x, n, (int)as_flag, bsum);
    PRIMX_CHECK_LAUNCH(name);
    PRIMX_TRY(scan_blocks(bsum, nblk, tot, st, name));
    hipLaunchKernelGGL(place_kernel, dim3(nblk), dim3(THREADS), 0, st, x, n, (int)as_flag, (const long long*)bsum, out, out2);
    PRIMX_CHECK_LAUNCH(name);
    return PRIMX_OK;
}

// device -> host on the stream, then wait for it
inline int readback(void* host, const void* dev, size_t bytes, hipStream_t st, const char* name) {
    if (hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        primx_set_error("%s: reading back from the device failed", name);
        return PRIMX_ELAUNCH;
    }
    return PRIMX_OK;
}

// The workspace of cleanup and decimation: REGIONS int arrays of M entries, the block sums of M items, PAIRS pairs of
// totals, FLAGS change flags, 8 ints.
template <int REGIONS, int PAIRS, int FLAGS>
struct MeshWs {
    char* w = nullptr;
    size_t region[REGIONS], bsum_at, tot_at, flags_at, small_at, total;
    explicit MeshWs(int64_t M = 1) {
        Arena a;
        for (size_t& r : region) r = a.take((size_t)M * 4);
        bsum_at = a.take((size_t)nblocks(M, PTS) * 16);
        tot_at = a.take(PAIRS * 16);
        flags_at = a.take(FLAGS * 4);
        small_at = a.take(8 * 4);
        total = a.total;
    }
    int* R(int r) const { return (int*)(w + region[r]); }
    long long* bsum() const { return (long long*)(w + bsum_at); }
    long long* tot(int k) const { return (long long*)(w + tot_at) + 2 * k; }
    int* flags() const { return (int*)(w + flags_at); }
    int* small() const { return (int*)(w + small_at); }
};

template <int REGIONS, int PAIRS, int FLAGS>
int check_ws(const char* name, int64_t M, const void* ws, int64_t ws_bytes, MeshWs<REGIONS, PAIRS, FLAGS>& out) {
    PRIMX_REQUIRE(ws, "%s: null pointer", name);
    out = MeshWs<REGIONS, PAIRS, FLAGS>(M);
    out.w = (char*)ws;
    PRIMX_REQUIRE(ws_bytes >= (int64_t)out.total, "%s: workspace of %lld bytes, need %lld", name, (long long)ws_bytes,
                  (long long)out.total);
    return PRIMX_OK;
}
