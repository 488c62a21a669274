// Block-prefix compaction and the one-workgroup scan shared by texbake.hip and meshclean.hip: a kernel counts its items
// per block of PTS (block_sums), tb_scan_kernel turns the block sums into exclusive offsets plus totals, and a second
// kernel walks the same blocks in the same order and places each item at offset + block_prefix.  Include inside the
// translation unit's anonymous namespace.
#pragma once

constexpr int THREADS = 256;
constexpr int ROUNDS = 4;
constexpr int PTS = THREADS * ROUNDS;   // items per block of the block-prefix kernels
constexpr int SCAN_THREADS = 1024;

__device__ __forceinline__ int lanes_below(unsigned long long m) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// Exclusive prefix of a 0 / 1 flag over the block's 256 threads in thread order; `total` = the block's sum.  Every
// thread of the block calls it.
__device__ __forceinline__ int block_prefix(bool c, int* s_wave, int& total) {
    const unsigned long long b = __ballot(c);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) s_wave[wave] = __popcll(b);
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) {
        off += (w < wave) ? s_wave[w] : 0;
        tot += s_wave[w];
    }
    __syncthreads();
    total = tot;
    return off + lanes_below(b);
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

// One workgroup: exclusive block offsets of both counters in place, totals [2] = the sums.
__global__ __launch_bounds__(SCAN_THREADS) void tb_scan_kernel(long long* __restrict__ bsum, int nblk,
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
