// Packed streams on the device: what the post-processors of packed audio (join.hip, master.hip, marks.hip, window.hip) do before they
// touch a sample.  (resample.hip keeps the same scheme written out in its kernel: with the shared search that kernel measured about 1 %
// slower at one ratio or another, for no reason its registers or LDS show.)  The streams' lengths exist on the device only -- in_off [G + 1], clamped to [0, in_cap] wherever it is
// read -- so a grid is sized by the capacity and every workgroup finds its own work:
//
//   find_job   a stream of n samples takes rows(n) rows of a table and items(n, its rows) workgroups.  Thread t sums both over its run of
//              ceil(G / TH) consecutive streams, an inclusive block scan turns the sums into prefixes, every thread walks its run again from
//              its prefix, and the thread whose run holds workgroup w publishes the stream through shared memory.  The walk can call a
//              visitor with every stream's prefixes (out_off and the like are stored there: no second pass).
//   behind     the workgroups behind the last item write the zeros from the last sample up to the capacity (fill_tail).
#pragma once
#include "common.h"
#include "artspeech_hip.h"

namespace packed_streams {

// the length of stream b and (*first) its first sample, inside [0, in_cap] whatever the offsets say
__device__ __forceinline__ int len_at(const int* in_off, int in_cap, int b, int* first)
{
    const int a = min(max(in_off[b], 0), in_cap), e = min(max(in_off[b + 1], 0), in_cap);
    *first = a;
    return max(e - a, 0);
}

// inclusive block scans over TH values, in place in the caller's shared arrays; the sums of scan_sum advance in step
template <int TH, class... T>
__device__ __forceinline__ void scan_sum(int t, T*... s)
{
    __syncthreads();
    for (int off = 1; off < TH; off <<= 1) {
        auto step = [&](T... v) {
            __syncthreads();
            ((s[t] += v), ...);
            __syncthreads();
        };
        step((t >= off ? s[t - off] : T(0))...);
    }
}
template <int TH>
__device__ __forceinline__ void scan_max(int t, int* s)            // of values >= -1
{
    __syncthreads();
    for (int off = 1; off < TH; off <<= 1) {
        const int v = t >= off ? s[t - off] : -1;
        __syncthreads();
        s[t] = max(s[t], v);
        __syncthreads();
    }
}

template <class TI, class TR>
struct Job {
    int first, n, idx;          // the stream's first sample and length, the workgroup's index among the stream's workgroups
    int own;                    // the stream's own rows (rows(n): nobody has to work it out a third time)
    TR base;                    // the table rows of the streams in front of it
    TI items;                   // totals over all streams
    TR rows;
};

// Workgroup w's stream among G, by TH threads.  false: w lies behind the last item (job->items and job->rows are set either way).
// visit(b, first, n, items_before, rows_before) is called once per stream by the thread that owns it.  TI / TR: the types the two sums are
// kept in -- they size the shared arrays, TH (sizeof(TI) + sizeof(TR)) bytes.  CALL ONCE PER KERNEL: the shared words belong to the
// instantiation and there is no barrier behind the last read, so a second call would race with the first one's readers.
template <int TH, class TI, class TR, class Items, class Rows, class Visit>
__device__ __forceinline__ bool find_job(int G, const int* __restrict__ in_off, int in_cap, TI w, Items items, Rows rows, Job<TI, TR>* job, Visit visit)
{
    __shared__ TI s_items[TH];
    __shared__ TR s_rows[TH];
    __shared__ TR s_base;
    __shared__ int s_job[4];
    __shared__ int s_found;
    const int t = threadIdx.x;
    if (t == 0) s_found = 0;
    const int per = (G + TH - 1) / TH, lo = min(t * per, G), hi = min(lo + per, G);
    TI li = 0;
    TR lr = 0;
    for (int b = lo; b < hi; ++b) {
        int first;
        const int n = len_at(in_off, in_cap, b, &first), own = rows(n);
        li += items(n, own);
        lr += own;
    }
    s_items[t] = li;
    s_rows[t] = lr;
    scan_sum<TH>(t, s_items, s_rows);
    TI ip = s_items[t] - li;
    TR rp = s_rows[t] - lr;
    for (int b = lo; b < hi; ++b) {
        int first;
        const int n = len_at(in_off, in_cap, b, &first), own = rows(n);
        const TI it = items(n, own);
        visit(b, first, n, ip, rp);
        if (w >= ip && w < ip + it) {
            s_base = rp;
            s_job[0] = first;
            s_job[1] = n;
            s_job[2] = (int)(w - ip);
            s_job[3] = own;
            s_found = 1;
        }
        ip += it;
        rp += own;
    }
    __syncthreads();
    job->first = s_job[0];
    job->n = s_job[1];
    job->idx = s_job[2];
    job->own = s_job[3];
    job->base = s_base;
    job->items = s_items[TH - 1];
    job->rows = s_rows[TH - 1];
    return s_found != 0;
}
template <int TH, class TI, class TR, class Items, class Rows>
__device__ __forceinline__ bool find_job(int G, const int* __restrict__ in_off, int in_cap, TI w, Items items, Rows rows, Job<TI, TR>* job)
{
    return find_job<TH>(G, in_off, in_cap, w, items, rows, job, [](int, int, int, TI, TR) {});
}

// the table rows in front of stream b, by one wave
template <class Rows>
__device__ __forceinline__ long long rows_before(int b, const int* __restrict__ in_off, int in_cap, int lane, Rows rows)
{
    long long base = 0;
    for (int j = lane; j < b; j += AS_WAVE) {
        int first;
        base += rows(len_at(in_off, in_cap, j, &first));
    }
    return as_wave_sum(base);
}

// one sample to wherever it goes: fp32 and / or 16-bit PCM (as_pcm16; a NaN stores 0 there and raises AS_STATUS_F16_RANGE)
__device__ __forceinline__ void put(float v, long long o, float* __restrict__ y, short* __restrict__ pcm, unsigned* status)
{
    if (y) y[o] = v;
    if (pcm) {
        bool nan;
        pcm[o] = (short)as_pcm16(v, &nan);
        if (nan) as_status_raise(status, AS_STATUS_F16_RANGE);
    }
}

// behind the last item: zeros over [from, cap), one tile's width per workgroup; idx = the workgroup's index behind the last item
template <int TH>
__device__ __forceinline__ void fill_tail(float* __restrict__ y, short* __restrict__ pcm, long long from, long long cap, long long idx, int width, int t)
{
    if (idx < 0) return;
    const long long z0 = from + idx * width, z1 = min(z0 + width, cap);
    for (long long o = z0 + t; o < z1; o += TH) {
        if (y) y[o] = 0.f;
        if (pcm) pcm[o] = 0;
    }
}

}  // namespace packed_streams
