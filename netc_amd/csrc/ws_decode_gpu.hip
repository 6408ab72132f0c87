// Receive-side frame decode for gfx950 (include/ws/frame.h, netc_gpu_decode_frames): the
// inverse of the frame assembly (ws_frame_gpu.hip).  The frames a netc_gpu_scan_frames call
// recorded in a wire stream become a mask.h batch -- payloads unmasked and packed back to
// back, n + 1 payload offsets -- plus a message table, all on the device, out of place.
//
// Two launches:
//   1. decode_offsets: one chained single-pass scan (decoupled look-back, gpu_util.h) over
//      the frames.  It carries three things per frame: the payload-length prefix (the
//      offsets), the count of FIN frames before it (the message index) and the last non-zero
//      opcode since the last FIN (the message's opcode so far; an associative segmented
//      operator, msg_combine).  The thread of a FIN frame writes its message's row.
//   2. decode_gather: destination-driven.  One wavefront per 4 KiB chunk of the payload
//      buffer, in 16-byte vectors aligned to the destination.  A vector inside one frame is
//      one unaligned 16-byte load from the wire, an XOR with the rotated key and one aligned
//      non-temporal store; every other vector (one that straddles a frame boundary, the
//      buffer's partial first and last vectors, a vector past the chunk's 64-entry frame
//      table) is composed byte by byte by its lane and written with byte stores, so no byte
//      outside [0, BYTES) is ever written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "gpu_util.h"
#include "ws_decode_gpu.h"
#include "ws_mask_gpu.h"
#include "../../include/ws/frame.h"

namespace netc_gpu {

namespace {

constexpr int kDecThreads = 256;                      // one frame per thread: every load is coalesced
constexpr int kDecWaves = kDecThreads / kWave;
constexpr uint64_t kChunk = 4096;                     // destination bytes per wavefront
constexpr int kChunkVecs = (int)(kChunk / kSpan);     // 16-byte vectors per lane and chunk
typedef uint32_t u32x4u __attribute__((ext_vector_type(4), aligned(1)));

// ------------------------------------------------------------ launch 1 -------

struct OffArgs {
    const uint8_t* wire;
    const uint64_t* hdr;
    const uint8_t* b0;
    const uint64_t* result;
    uint64_t max_frames;
    uint64_t len;
    uint64_t* offsets;
    uint64_t* msg_first;
    uint8_t* msg_opcode;
    uint64_t* dresult;
    uint64_t* st_bytes;   // status words of the payload-length scan (gpu_util.h layout)
    uint64_t* st_msg;     // ... of the message scan: [63:62] flag | [61:46] epoch | [45:42] opcode | [41:0] FINs
    uint32_t epoch;
};

// Message state of a run of frames: FINs in it << 4 | the last non-zero opcode after its last
// FIN (0: none).  One frame: 1 << 4 for a FIN frame (its message is closed: nothing carries
// on), its opcode otherwise.  0 is the identity.
__device__ __forceinline__ uint64_t msg_combine(uint64_t a, uint64_t b) {
    const uint64_t op = (b >> 4) != 0 || (b & 15) != 0 ? (b & 15) : (a & 15);
    return (((a >> 4) + (b >> 4)) << 4) | op;
}

constexpr uint64_t kFinBits = 42;
constexpr uint64_t kFinMask = (1ull << kFinBits) - 1;

__device__ __forceinline__ uint64_t msg_word(uint64_t flag, uint32_t epoch, uint64_t state) {
    return flag << 62 | (uint64_t)(epoch & 0xFFFF) << kValBits | (state & 15) << kFinBits | ((state >> 4) & kFinMask);
}

// look_back (gpu_util.h) for the message state: the FIN counts of the predecessors add up as
// there; the opcode is that of the nearest predecessor that decides it -- an aggregate with a
// non-zero opcode or a FIN (opcode 0 after a FIN: nothing carries over), or the inclusive
// prefix the walk stops at.
__device__ inline uint64_t look_back_msg(uint64_t* status, int64_t tile, uint32_t epoch, int lane) {
    uint64_t fins = 0;
    uint32_t op = 0;
    bool open = true;   // the opcode is not decided yet (uniform)
    for (int64_t top = tile - 1; top >= 0;) {
        const int64_t idx = top - lane;
        uint64_t f = 0;
        uint32_t o = 0;
        bool ok = true, incl = idx < 0;   // before tile 0: an inclusive prefix of nothing
        if (idx >= 0) {
            const uint64_t w = __hip_atomic_load(&status[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            ok = (w >> 62) != 0 && ((w >> kValBits) & 0xFFFF) == (epoch & 0xFFFF);
            incl = ok && (w >> 62) == 2;
            f = w & kFinMask;
            o = (uint32_t)(w >> kFinBits) & 15u;
        }
        const uint64_t im = __ballot(incl);
        const int stop = im ? __builtin_ctzll(im) : kWave;
        const uint64_t need = stop >= kWave - 1 ? ~0ull : ((2ull << stop) - 1);
        if ((__ballot(ok) & need) != need) {
            __builtin_amdgcn_s_sleep(1);
            continue;
        }
        const bool in = lane <= stop;
        fins += wave_sum(in ? f : 0);
        if (open) {
            const uint64_t dm = __ballot(in && (o != 0 || f != 0 || incl));
            if (dm) {
                op = readlane32(o, __builtin_ctzll(dm));
                open = false;
            }
        }
        if (stop < kWave) break;
        top -= kWave;
    }
    return fins << 4 | op;
}

__global__ __launch_bounds__(kDecThreads) void decode_offsets(OffArgs a) {
    __shared__ uint64_t wave_bytes[kDecWaves], wave_msg[kDecWaves], tile_bytes, tile_msg;
    const uint64_t found = a.len >= 2 ? gptr(a.result)[NETC_WS_SCAN_FRAMES] : 0;
    const uint64_t n = found < a.max_frames ? found : a.max_frames;
    const uint64_t tile = blockIdx.x, k = tile * kDecThreads + threadIdx.x;
    if (n == 0) {
        if (tile == 0 && threadIdx.x == 0) {
            gptr(a.offsets)[0] = 0;
            if (a.msg_first) gptr(a.msg_first)[0] = 0;
            gptr(a.dresult)[NETC_WS_DECODE_FRAMES] = 0;
            gptr(a.dresult)[NETC_WS_DECODE_BYTES] = 0;
            gptr(a.dresult)[NETC_WS_DECODE_MESSAGES] = 0;
        }
        return;
    }
    if (tile * kDecThreads >= n) return;   // the grid is sized for max_frames
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const bool valid = k < n;
    // loads at clamped indices, the values of frames past n dropped afterwards
    const uint64_t kc = valid ? k : n - 1;
    const uint64_t p = gptr(a.hdr)[kc], pn = gptr(a.hdr)[kc + 1];   // hdr holds max_frames + 1 >= n + 1 entries
    const uint32_t first = gptr(a.b0)[kc];
    const uint32_t second = gptr(a.wire)[p + 1];
    const uint32_t code = second & 0x7F;
    const uint64_t hl = 2 + (code == 126 ? 2 : (code == 127 ? 8 : 0)) + ((second & 0x80) ? 4 : 0);
    uint64_t flen = pn - p - hl;
    if (kc == n - 1 && found > a.max_frames) {
        // max_frames cut the record short: hdr[n] was not written, the length is in the header
        flen = code;
        if (code >= 126) {
            flen = 0;
            for (int j = 0; j < (code == 126 ? 2 : 8); ++j) flen = flen << 8 | gptr(a.wire)[p + 2 + j];
        }
    }
    if (!valid) flen = 0;
    const bool fin = valid && (first & 0x80);
    const uint32_t opcode = first & 0x0F;
    const uint64_t mine = !valid ? 0 : (fin ? 1ull << 4 : (uint64_t)opcode);

    // inclusive scans inside the wavefront, then across the block's wavefronts
    uint64_t ib = flen, im = mine;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const uint64_t yb = (uint64_t)__shfl_up((unsigned long long)ib, d, kWave);
        const uint64_t ym = (uint64_t)__shfl_up((unsigned long long)im, d, kWave);
        if (lane >= d) {
            ib += yb;
            im = msg_combine(ym, im);
        }
    }
    if (lane == kWave - 1) {
        wave_bytes[wave] = ib;
        wave_msg[wave] = im;
    }
    __syncthreads();
    uint64_t pre_b = 0, pre_m = 0, agg_b = 0, agg_m = 0;   // this wavefront's prefix, the tile's aggregate
#pragma unroll
    for (int w = 0; w < kDecWaves; ++w) {
        if (w == wave) {
            pre_b = agg_b;
            pre_m = agg_m;
        }
        agg_b += wave_bytes[w];
        agg_m = msg_combine(agg_m, wave_msg[w]);
    }
    // wavefront 0 chains the payload bytes, wavefront 1 the message state
    if (wave == 0) {
        if (lane == 0)
            __hip_atomic_store(&a.st_bytes[tile], status_word(tile == 0 ? 2 : 1, a.epoch, agg_b), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        const uint64_t prefix = tile == 0 ? 0 : look_back(a.st_bytes, (int64_t)tile, a.epoch, lane);
        if (lane == 0) {
            if (tile)
                __hip_atomic_store(&a.st_bytes[tile], status_word(2, a.epoch, prefix + agg_b), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            tile_bytes = prefix;
        }
    } else if (wave == 1) {
        if (lane == 0)
            __hip_atomic_store(&a.st_msg[tile], msg_word(tile == 0 ? 2 : 1, a.epoch, agg_m), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        const uint64_t prefix = tile == 0 ? 0 : look_back_msg(a.st_msg, (int64_t)tile, a.epoch, lane);
        if (lane == 0) {
            if (tile)
                __hip_atomic_store(&a.st_msg[tile], msg_word(2, a.epoch, msg_combine(prefix, agg_m)), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            tile_msg = prefix;
        }
    }
    __syncthreads();
    const uint64_t end_b = tile_bytes + pre_b + ib;                               // offsets[k + 1]
    const uint64_t end_m = msg_combine(msg_combine(tile_msg, pre_m), im);          // state after frame k
    // the state before frame k: the lane below's, or the wavefront's prefix
    uint64_t eb = (uint64_t)__shfl_up((unsigned long long)ib, 1, kWave);
    uint64_t em = (uint64_t)__shfl_up((unsigned long long)im, 1, kWave);
    if (lane == 0) eb = 0, em = 0;
    const uint64_t beg_m = msg_combine(msg_combine(tile_msg, pre_m), em);
    if (!valid) return;
    gptr(a.offsets)[k] = tile_bytes + pre_b + eb;
    if (a.msg_first) {
        if (k == 0) gptr(a.msg_first)[0] = 0;
        if (fin) {
            const uint64_t m = beg_m >> 4;
            gptr(a.msg_first)[m + 1] = k + 1;
            gptr(a.msg_opcode)[m] = (uint8_t)(opcode ? opcode : (uint32_t)(beg_m & 15));
        }
        // msg_first[M] is the open message's first frame already: the row its predecessor's FIN
        // wrote (or row 0), and n when the last frame has FIN
    }
    if (k == n - 1) {
        gptr(a.offsets)[n] = end_b;
        gptr(a.dresult)[NETC_WS_DECODE_FRAMES] = n;
        gptr(a.dresult)[NETC_WS_DECODE_BYTES] = end_b;
        gptr(a.dresult)[NETC_WS_DECODE_MESSAGES] = end_m >> 4;
    }
}

// ------------------------------------------------------------ launch 2 -------

struct GatherArgs {
    uint8_t* dst_base;         // payload rounded down to 16 B
    uint64_t mis;              // payload & 15: payload byte q is dst_base[mis + q]
    const uint8_t* wire;
    uint64_t len;
    const uint64_t* hdr;
    const uint32_t* keys;
    const uint64_t* offsets;   // launch 1's output
    const uint64_t* dresult;   // ... frames and bytes
};

// Payload bytes [q, qe) composed by one lane, frame by frame from frame k, the last frame
// whose offset is <= q (search: k is only a lower bound of it).  Byte stores only.
__device__ __forceinline__ void compose_bytes(const GatherArgs& a, uint64_t k, uint64_t q, uint64_t qe, uint64_t n,
                                           bool search) {
    const NETC_GLOBAL uint64_t* off = gptr(a.offsets);
    if (search) {
        uint64_t lo = k, hi = n;   // off[lo] <= q < off[hi]
        while (hi - lo > 1) {
            const uint64_t mid = lo + ((hi - lo) >> 1);
            if (off[mid] <= q) lo = mid;
            else hi = mid;
        }
        k = lo;
    }
    NETC_GLOBAL uint8_t* dst = gptr(a.dst_base) + a.mis;
    while (q < qe && k < n) {
        const uint64_t o1 = off[k + 1];
        if (o1 <= q) {   // an empty frame, or one that ends before q
            ++k;
            continue;
        }
        const uint64_t o0 = off[k], p = gptr(a.hdr)[k];
        const uint32_t key = gptr(a.keys)[k];
        const uint32_t second = gptr(a.wire)[p + 1];
        const uint32_t code = second & 0x7F;
        const uint64_t hl = 2 + (code == 126 ? 2 : (code == 127 ? 8 : 0)) + ((second & 0x80) ? 4 : 0);
        const NETC_GLOBAL uint8_t* src = gptr(a.wire) + p + hl;
        const uint64_t e = o1 < qe ? o1 : qe;
        for (; q < e; ++q) {
            const uint64_t i = q - o0;
            dst[q] = (uint8_t)(src[i] ^ (uint8_t)(key >> (8 * (i & 3))));
        }
        ++k;
    }
}

__global__ __launch_bounds__(kDecThreads) void decode_gather(GatherArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const uint64_t chunk = (uint64_t)blockIdx.x * kDecWaves + (uint64_t)__builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const uint64_t n = gptr(a.dresult)[NETC_WS_DECODE_FRAMES], total = gptr(a.dresult)[NETC_WS_DECODE_BYTES];
    // payload coordinate of the chunk's first byte (negative in chunk 0 of a misaligned buffer)
    const int64_t qb = (int64_t)(chunk * kChunk) - (int64_t)a.mis;
    if (n == 0 || total == 0 || qb >= (int64_t)total) return;   // uniform
    const uint64_t q0 = qb < 0 ? 0 : (uint64_t)qb;

    // kb: the last frame whose offset is <= q0 (an upper-bound search, so that a run of empty
    // frames at q0 resolves to the frame that owns the byte), 64 probes per step
    const NETC_GLOBAL uint64_t* off = gptr(a.offsets);
    uint64_t lo = 0, hi = n;   // off[lo] <= q0 < off[hi]
    while (hi - lo > 1) {
        const uint64_t step = (hi - lo + 63) >> 6;
        uint64_t idx = lo + (uint64_t)(lane + 1) * step;
        if (idx > hi) idx = hi;
        const int cnt = __popcll(__ballot(off[idx] <= q0));   // the probes are sorted: a prefix of the lanes
        const uint64_t nlo = lo + (uint64_t)cnt * step;
        uint64_t nhi = lo + (uint64_t)(cnt + 1) * step;
        if (nhi > hi) nhi = hi;
        lo = nlo;
        hi = nhi;
    }
    const uint64_t kb = lo;

    // the chunk's frame table: lane l holds frame kb + l
    constexpr int64_t kFar = 1ll << 30;
    const uint64_t ti = kb + (uint64_t)lane;
    const uint64_t tio = ti <= n ? ti : n, tif = ti < n ? ti : n - 1;
    const uint64_t st = off[tio], hp = gptr(a.hdr)[tif];
    const uint32_t ky = gptr(a.keys)[tif];
    const uint32_t second = gptr(a.wire)[hp + 1];
    const uint32_t code = second & 0x7F;
    const uint64_t hl = 2 + (code == 126 ? 2 : (code == 127 ? 8 : 0)) + ((second & 0x80) ? 4 : 0);
    int64_t rel64 = ti <= n ? (int64_t)st - qb : kFar;   // the frame's offset relative to the chunk, saturated
    rel64 = rel64 < -kFar ? -kFar : (rel64 > kFar ? kFar : rel64);
    const int rel = (int)rel64;
    const uint64_t sadj = hp + hl - st;                           // payload byte q is wire[sadj + q]
    const uint32_t kadj = rotr8(ky, (4 - (st & 3)) & 3);          // its key byte is that of rotr8(kadj, q)
    const int rel0 = __builtin_amdgcn_readfirstlane(rel);

    int tt[kChunkVecs];
    bool fast[kChunkVecs], live[kChunkVecs];
    uint32_t kk[kChunkVecs];
    u32x4 d[kChunkVecs];
    const bool safe16 = a.len >= 16;
#pragma unroll
    for (int it = 0; it < kChunkVecs; ++it) {
        const int qr = it * (int)kSpan + lane * 16;     // the vector is [qr, qr + 16) of the chunk
        const int64_t q = qb + qr;
        live[it] = q < (int64_t)total && q + 16 > 0;
        const int qs = q < 0 ? (int)(0 - qb) : qr;      // its first byte inside the buffer
        int t = 0, rt = rel0;
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {              // the last entry at or before qs (entry 0 always is)
            const int v = __builtin_amdgcn_ds_bpermute((t + s) << 2, rel);
            if (v <= qs) {
                t += s;
                rt = v;
            }
        }
        const int re = __builtin_amdgcn_ds_bpermute((t < 63 ? t + 1 : 63) << 2, rel);
        const uint64_t sa = bperm64(sadj, t);
        kk[it] = (uint32_t)__builtin_amdgcn_ds_bpermute(t << 2, (int)kadj);
        tt[it] = t;
        // one frame holds the whole vector (entry 63's end is not in the table: composed)
        fast[it] = live[it] && safe16 && t < 63 && q >= 0 && rt <= qr && qr + 16 <= re;
        d[it] = u32x4{0, 0, 0, 0};
        if (safe16) {   // straight-line loads: a lane without one reads the stream's first bytes
            const uint8_t* src = fast[it] ? a.wire + (sa + (uint64_t)q) : a.wire;
            d[it] = *(const NETC_GLOBAL u32x4u*)src;
        }
    }
#pragma unroll
    for (int it = 0; it < kChunkVecs; ++it) {
        const int qr = it * (int)kSpan + lane * 16;
        const int64_t q = qb + qr;
        if (fast[it]) {
            const uint32_t rk = rotr8(kk[it], (uint64_t)q);
            const u32x4 kv = {rk, rk, rk, rk};
            __builtin_nontemporal_store(d[it] ^ kv, (NETC_GLOBAL u32x4*)(a.dst_base + chunk * kChunk + (uint64_t)qr));
        }
    }
#pragma unroll 1
    for (int it = 0; it < kChunkVecs; ++it) {
        const int qr = it * (int)kSpan + lane * 16;
        const int64_t q = qb + qr;
        const bool f = it == 0 ? fast[0] : it == 1 ? fast[1] : it == 2 ? fast[2] : fast[3];
        const bool l = it == 0 ? live[0] : it == 1 ? live[1] : it == 2 ? live[2] : live[3];
        const int t = it == 0 ? tt[0] : it == 1 ? tt[1] : it == 2 ? tt[2] : tt[3];
        if (l && !f) {
            const uint64_t qlo = q < 0 ? 0 : (uint64_t)q;
            const uint64_t qhi = (uint64_t)(q + 16) < total ? (uint64_t)(q + 16) : total;
            compose_bytes(a, kb + (uint64_t)t, qlo, qhi, n, t == 63);
        }
    }
}

// ------------------------------------------------------------- scratch -------

// Per (device, stream): the two status arrays of launch 1, one word per tile each.  Work
// queued on one stream runs in order and shares them (the epoch tells calls apart); an
// outgrown array may still be read by work queued before the growth, so it is kept until
// release_dec_scratch.
struct DecScratch {
    uint64_t* status = nullptr;   // [0, tiles): payload bytes, [tiles, 2 tiles): messages
    uint64_t tiles = 0;
    uint32_t epoch = 0;
    std::vector<void*> retired;
};

std::map<std::pair<int, hipStream_t>, DecScratch> g_dec;
std::mutex g_dec_mu;

hipError_t dec_scratch_for(hipStream_t stream, uint64_t tiles, DecScratch& out) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> g(g_dec_mu);
    DecScratch& sc = g_dec[{dev, stream}];
    if (sc.tiles < tiles) {
        uint64_t* p = nullptr;
        uint64_t want = sc.tiles ? 2 * sc.tiles : 1024;
        while (want < tiles) want *= 2;
        if ((e = hipMalloc(&p, 2 * want * sizeof(uint64_t))) != hipSuccess) return e;
        if ((e = hipMemsetAsync(p, 0, 2 * want * sizeof(uint64_t), stream)) != hipSuccess) {
            (void)hipFree(p);
            return e;
        }
        if (sc.status) sc.retired.push_back(sc.status);
        sc.status = p;
        sc.tiles = want;
        sc.epoch = 0;
    }
    sc.epoch = (sc.epoch + 1) & 0xFFFF;
    if (sc.epoch == 0) {   // epochs wrapped: clear the words so no stale epoch can match
        if ((e = hipMemsetAsync(sc.status, 0, 2 * sc.tiles * sizeof(uint64_t), stream)) != hipSuccess) return e;
        sc.epoch = 1;
    }
    out.status = sc.status;
    out.tiles = sc.tiles;
    out.epoch = sc.epoch;
    return hipSuccess;
}

}  // namespace

int release_dec_scratch(int device, hipStream_t stream) {
    DecScratch sc;
    {
        std::lock_guard<std::mutex> g(g_dec_mu);
        auto it = g_dec.find({device, stream});
        if (it == g_dec.end()) return 0;
        sc = std::move(it->second);
        g_dec.erase(it);
    }
    if (sc.status) (void)hipFree(sc.status);
    for (void* p : sc.retired) (void)hipFree(p);
    return 1;
}

hipError_t launch_decode_frames(uint8_t* payload, uint64_t* offsets, uint64_t* msg_first, uint8_t* msg_opcode,
                                uint64_t* dresult, const uint8_t* wire, uint64_t len, const uint64_t* hdr,
                                const uint32_t* keys, const uint8_t* b0, uint64_t max_frames, const uint64_t* result,
                                hipStream_t stream) {
    // a frame is 2 bytes at least: the grid is sized for the frames max_frames and len allow
    const uint64_t cap = max_frames < len / 2 ? max_frames : len / 2;
    const uint64_t tiles = cap / kDecThreads + 1;
    DecScratch sc;
    hipError_t e = dec_scratch_for(stream, tiles, sc);
    if (e != hipSuccess) return e;
    OffArgs oa;
    oa.wire = wire;
    oa.hdr = hdr;
    oa.b0 = b0;
    oa.result = result;
    oa.max_frames = cap;
    oa.len = len;
    oa.offsets = offsets;
    oa.msg_first = msg_first;
    oa.msg_opcode = msg_opcode;
    oa.dresult = dresult;
    oa.st_bytes = sc.status;
    oa.st_msg = sc.status + sc.tiles;
    oa.epoch = sc.epoch;
    hipLaunchKernelGGL(decode_offsets, dim3((unsigned)tiles), dim3(kDecThreads), 0, stream, oa);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (len < 2) return hipSuccess;   // no frame: nothing to gather
    GatherArgs ga;
    ga.mis = (uint64_t)((uintptr_t)payload & 15);
    ga.dst_base = payload - ga.mis;
    ga.wire = wire;
    ga.len = len;
    ga.hdr = hdr;
    ga.keys = keys;
    ga.offsets = offsets;
    ga.dresult = dresult;
    const uint64_t chunks = (ga.mis + len + kChunk - 1) / kChunk;   // the payload is shorter than the stream
    hipLaunchKernelGGL(decode_gather, dim3((unsigned)((chunks + kDecWaves - 1) / kDecWaves)), dim3(kDecThreads), 0,
                       stream, ga);
    return hipGetLastError();
}

}  // namespace netc_gpu
