// Host code shared by the rings and hubs (ws_ingest.hip, ws_hub.hip, ws_egress.hip,
// ws_egress_hub.hip) and the C-ABI layer (ws_mask_api.hip).  Internal, not installed; host only
// -- no kernel, no device function.  Everything is inline with internal linkage: the
// per-message paths still inline into their callers and the libraries export nothing new.
//
//   DeviceGuard                 the calling thread's device for a scope
//   SockId                      a socket's identity against descriptor reuse
//   SendSlot, SendLayout        one slot of a send ring: fill, submit (H2D, frame assembly, D2H)
//   PeekSock                    a socket read ahead with MSG_PEEK: peek, consume, the ERECV report
//   MsgBuf                      frames reassembled into a message (the reference's rules)
//
// What differs between the users stays with them: the ring's FIFO and hand-out, the hubs' spans,
// ranges, generations and statistics, when a route releases its hostage byte.
#pragma once

#include <hip/hip_runtime.h>

#include <errno.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/socket.h>
#include <sys/stat.h>
#include <sys/uio.h>

#include "ws_mask_gpu.h"

extern "C" {
#include "../../include/ws/mask.h"
#include "../../include/ws/frame.h"
#include "../../include/ws/ingest.h"
#include "../../include/ws/common.h"
#include "host/ws_header.h"
extern __thread int netc_errno_reason;   // include/utils/error.h
}

namespace {

// Selects `device` for the calling thread for the lifetime of the guard.  The hot
// path (the device is already current) costs one hipGetDevice (a thread-local read
// in the runtime) and nothing on exit.
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int device) {
        err = hipGetDevice(&prev);
        if (err != hipSuccess || prev == device) return;
        err = hipSetDevice(device);
        switched = err == hipSuccess;
    }
    ~DeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
};

// `who` ("egress", "hub", ...) in front of a HIP failure's text
inline int ring_fail_hip(int code, const char* who, const char* what, hipError_t e) {
    char text[96];
    snprintf(text, sizeof text, "%s: %s", who, what);
    return netc_gpu::api_fail_hip(code, text, e);
}

// ---------------------------------------------------------------- socket identity --

// the identity of an open socket (device, inode), to tell a reused descriptor from the attached one
struct SockId {
    uint64_t dev = 0, ino = 0;
};

inline bool sock_identity(int fd, SockId* id) {
    struct stat st;
    if (fstat(fd, &st) != 0 || !S_ISSOCK(st.st_mode)) return false;
    id->dev = (uint64_t)st.st_dev;
    id->ino = (uint64_t)st.st_ino;
    return true;
}

inline bool operator==(const SockId& a, const SockId& b) { return a.dev == b.dev && a.ino == b.ino; }

// fd still names the socket `id` was taken from
inline bool same_socket(int fd, const SockId& id) {
    SockId now;
    return sock_identity(fd, &now) && now == id;
}

enum : int { kNotStream = -1, kStreamOther = 0, kStreamTcp = 1 };

// what the receive routes can attach: a stream socket, and whether it is TCP (PeekSock::tcp)
inline int stream_socket_kind(int fd) {
    int type = 0, domain = 0;
    socklen_t tl = sizeof type, dl = sizeof domain;
    if (getsockopt(fd, SOL_SOCKET, SO_TYPE, &type, &tl) != 0 || type != SOCK_STREAM) return kNotStream;
    (void)getsockopt(fd, SOL_SOCKET, SO_DOMAIN, &domain, &dl);
    return domain == AF_INET || domain == AF_INET6 ? kStreamTcp : kStreamOther;
}

// ---------------------------------------------------------------- the send-side slot --

struct SendLayout {
    uint64_t slot_bytes = 0, max_frames = 0, wire_cap = 0;
    uint64_t keys_at = 0, b0_at = 0;   // h_tab regions of the keys and header bytes while filling
};

inline SendLayout send_layout(uint64_t slot_bytes, uint64_t max_frames) {
    SendLayout l;
    l.slot_bytes = slot_bytes;
    l.max_frames = max_frames;
    l.wire_cap = slot_bytes + max_frames * NETC_WS_MAX_HEADER(1);
    l.keys_at = (max_frames + 1) * sizeof(uint64_t);
    l.b0_at = l.keys_at + max_frames * sizeof(uint32_t);
    return l;
}

struct SendSlot {
    uint8_t* h_pay = nullptr;     // pinned: queued payload bytes (slot_bytes)
    uint8_t* h_tab = nullptr;     // offsets [0, 8 (mf + 1)), keys and header bytes in their own
                                  // regions while filling
    uint8_t* h_pack = nullptr;    // pinned: the table packed at submit (offsets | keys | header
                                  // bytes), so a failed submission leaves h_tab intact for a retry
    uint8_t* h_wire = nullptr;    // pinned: the slot's wire bytes (D2H target)
    uint64_t* h_len = nullptr;    // pinned: the device's wire length (wo[n])
    uint8_t* d_pay = nullptr;
    uint8_t* d_tab = nullptr;
    uint8_t* d_wire = nullptr;
    uint64_t* d_wo = nullptr;     // wire offsets (n + 1)
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    int state = 0;                // the owner's SlotState
    int masked = -1;              // the slot's frames are masked (1) or not (0); -1 while empty
    int ext = -2;                 // the frames' extended-length bytes: one class (0, 2, 8), mixed (-1),
                                  // none yet (-2); one class: the assembly launches without its scan
    uint64_t fill = 0;            // payload bytes queued
    uint64_t frames = 0;
    uint64_t wire = 0;            // wire bytes of the queued frames
};

inline void send_slot_free(int device, SendSlot& s) {
    if (s.stream) {
        (void)hipStreamSynchronize(s.stream);
        (void)netc_gpu::release_enc_scratch(device, s.stream);   // the encoder's per-stream scratch
    }
    if (s.h_pay) (void)hipHostFree(s.h_pay);
    if (s.h_tab) (void)hipHostFree(s.h_tab);
    if (s.h_pack) (void)hipHostFree(s.h_pack);
    if (s.h_wire) (void)hipHostFree(s.h_wire);
    if (s.h_len) (void)hipHostFree(s.h_len);
    if (s.d_pay) (void)hipFree(s.d_pay);
    if (s.d_tab) (void)hipFree(s.d_tab);
    if (s.d_wire) (void)hipFree(s.d_wire);
    if (s.d_wo) (void)hipFree(s.d_wo);
    if (s.done) (void)hipEventDestroy(s.done);
    if (s.stream) (void)hipStreamDestroy(s.stream);
    s = SendSlot();
}

inline int send_slot_alloc(const SendLayout& l, SendSlot& s, const char* who) {
    hipError_t e;
    const uint64_t mf = l.max_frames, tab = l.b0_at + mf;
    if ((e = hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&s.done, hipEventDisableTiming)) != hipSuccess)
        return ring_fail_hip(NETC_GPU_ERUNTIME, who, "stream / event create", e);
    if ((e = hipHostMalloc((void**)&s.h_pay, l.slot_bytes, hipHostMallocDefault)) != hipSuccess ||
        (e = hipHostMalloc((void**)&s.h_tab, tab, hipHostMallocDefault)) != hipSuccess ||
        (e = hipHostMalloc((void**)&s.h_pack, tab, hipHostMallocDefault)) != hipSuccess ||
        (e = hipHostMalloc((void**)&s.h_wire, l.wire_cap, hipHostMallocDefault)) != hipSuccess ||
        (e = hipHostMalloc((void**)&s.h_len, sizeof(uint64_t), hipHostMallocDefault)) != hipSuccess)
        return ring_fail_hip(NETC_GPU_ENOMEM, who, "pinned host allocation", e);
    if ((e = hipMalloc((void**)&s.d_pay, l.slot_bytes)) != hipSuccess ||
        (e = hipMalloc((void**)&s.d_tab, tab)) != hipSuccess ||
        (e = hipMalloc((void**)&s.d_wire, l.wire_cap)) != hipSuccess ||
        (e = hipMalloc((void**)&s.d_wo, (mf + 1) * sizeof(uint64_t))) != hipSuccess)
        return ring_fail_hip(NETC_GPU_ENOMEM, who, "device allocation", e);
    return 0;
}

// One message into the filling slot: its payload (the one host copy) and its frames' table
// entries -- the reference's split (src/ws/common.c:42-49: equal parts, the remainder on the
// last), one key, header byte 0 per frame (:55-61).  The caller has checked that it fits.
// Returns the message's wire bytes (known on the host from the lengths).  Always inlined: it is
// the per-message path of both send rings, and out of line it cost the ring a quarter of its
// 1 KiB message rate.
__attribute__((always_inline)) inline uint64_t send_slot_append(SendSlot& s, const SendLayout& l, const void* payload, uint64_t len, uint8_t opcode,
                                 const uint8_t* masking_key, uint64_t nf) {
    const bool masked = masking_key != nullptr;
    s.masked = masked ? 1 : 0;
    if (len) memcpy(s.h_pay + s.fill, payload, len);
    const uint64_t split = len / nf, rem = len % nf;
    uint64_t* off = (uint64_t*)s.h_tab + s.frames;
    uint32_t* keys = (uint32_t*)(s.h_tab + l.keys_at) + s.frames;
    uint8_t* b0 = s.h_tab + l.b0_at + s.frames;
    const uint32_t key32 = masked ? (uint32_t)masking_key[0] | (uint32_t)masking_key[1] << 8 |
                                        (uint32_t)masking_key[2] << 16 | (uint32_t)masking_key[3] << 24
                                  : 0u;
    uint64_t wire = 0;
    for (uint64_t i = 0; i < nf; ++i) {
        const bool last = i + 1 == nf;
        const uint64_t flen = split + (last ? rem : 0);
        off[i] = s.fill + i * split;
        if (masked) keys[i] = key32;
        b0[i] = (uint8_t)((last ? 0x80 : 0x00) | (i == 0 ? (opcode & 0x0F) : WS_OPCODE_CONTINUE));
        wire += ws_header_len(flen, masked) + flen;
        const int ext = (int)ws_header_ext(flen);
        s.ext = s.ext == -2 || s.ext == ext ? ext : -1;
    }
    s.fill += len;
    s.frames += nf;
    s.wire += wire;
    return wire;
}

// The filled slot's GPU work, queued on its stream (the calling thread is on the slot's device):
//   H2D     the payload bytes, then the packed table (offsets | keys | header bytes: one copy)
//   encode  launch_encode_frames (ws_frame_gpu.hip): one launch when every frame of the slot is
//           in one length class (the host saw each length: the offsets are affine, no scan)
//   D2H     the wire bytes (the host summed the header lengths while queueing) and the device's
//           own wire length beside them, checked against it when the slot is taken; event "done"
inline int send_slot_submit(const SendLayout& l, SendSlot& s, const char* who) {
    const uint64_t n = s.frames;
    uint64_t* off = (uint64_t*)s.h_pack;
    uint8_t* keys = s.h_pack + (n + 1) * sizeof(uint64_t);
    uint8_t* b0 = keys + n * sizeof(uint32_t);
    const bool masked = s.masked == 1;
    memcpy(off, s.h_tab, n * sizeof(uint64_t));
    if (masked) memcpy(keys, s.h_tab + l.keys_at, n * sizeof(uint32_t));
    memcpy(b0, s.h_tab + l.b0_at, n);
    off[n] = s.fill;
    const uint64_t tab = (uint64_t)(b0 + n - s.h_pack);
    const uint64_t bound = s.fill + n * NETC_WS_MAX_HEADER(masked);
    hipError_t e;
    if ((s.fill && (e = hipMemcpyAsync(s.d_pay, s.h_pay, s.fill, hipMemcpyHostToDevice, s.stream)) != hipSuccess) ||
        (e = hipMemcpyAsync(s.d_tab, s.h_pack, tab, hipMemcpyHostToDevice, s.stream)) != hipSuccess)
        return ring_fail_hip(NETC_GPU_ERUNTIME, who, "H2D copy", e);
    const uint8_t* d_keys = s.d_tab + (n + 1) * sizeof(uint64_t);
    if ((e = netc_gpu::launch_encode_frames(s.d_wire, bound, s.d_pay, s.fill, (const uint64_t*)s.d_tab,
                                            (const uint32_t*)d_keys, d_keys + n * sizeof(uint32_t), n, masked,
                                            s.d_wo, s.stream, netc_gpu::api_cfg(), s.ext >= 0 ? s.ext : -1)) !=
        hipSuccess)
        return ring_fail_hip(e == hipErrorOutOfMemory ? NETC_GPU_ENOMEM : NETC_GPU_ELAUNCH, who, "frame assembly", e);
    *s.h_len = ~0ull;
    if ((e = hipMemcpyAsync(s.h_wire, s.d_wire, s.wire, hipMemcpyDeviceToHost, s.stream)) != hipSuccess ||
        (e = hipMemcpyAsync(s.h_len, s.d_wo + n, sizeof(uint64_t), hipMemcpyDeviceToHost, s.stream)) != hipSuccess ||
        (e = hipEventRecord(s.done, s.stream)) != hipSuccess)
        return ring_fail_hip(NETC_GPU_ERUNTIME, who, "D2H copy", e);
    return 0;
}

// ---------------------------------------------------------------- the peeked socket --

constexpr int kBadRecv = 10;                // netc's BADRECV reason (include/utils/error.h)
constexpr size_t kDiscardBytes = 1u << 20;  // discard buffer of non-TCP sockets

// A socket a receive route reads ahead of: bytes are copied out with MSG_PEEK and removed only
// up to sock_pos.  How far it has peeked (in_pos) is its owner's count.
struct PeekSock {
    int fd = -1;                 // attached socket, -1 = none
    SockId id;                   // its identity at attach time (fstat), against fd reuse
    int tcp = 0;                 // TCP: discard with MSG_TRUNC (no copy); else recv into scratch
    uint64_t sock_pos = 0;       // stream bytes removed from the socket
    uint8_t* scratch = nullptr;  // discard buffer for non-TCP sockets (malloc; the owner frees it)
};

// a failed recv: NETC_WS_INGEST_ERECV with "<what>: <strerror>", netc's BADRECV reason, errno kept
inline int recv_failed(int saved, const char* fmt, ...) {
    char what[128];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(what, sizeof what, fmt, ap);
    va_end(ap);
    netc_gpu::api_fail(NETC_WS_INGEST_ERECV, "%s: %s", what, strerror(saved));
    netc_errno_reason = kBadRecv;
    errno = saved;
    return NETC_WS_INGEST_ERECV;
}

// Peek up to `room` bytes past the `held` (0 or 1) the owner already has -- its hostage byte,
// still in the socket -- into dst; the held byte goes to a scratch byte.  Returns recvmsg's
// result, the held bytes counted in it: <= held is only what the owner has, 0 the peer's close,
// < 0 with errno for the caller.  MSG_DONTWAIT: a route peeks again after releasing its hostage,
// when the socket may hold nothing -- a blocking socket must not stall the caller's loop there.
inline ssize_t sock_peek(const PeekSock& ps, int held, uint8_t* dst, size_t room) {
    uint8_t skip[1];
    struct iovec iov[2] = {{skip, (size_t)held}, {dst, room}};
    struct msghdr mh;
    memset(&mh, 0, sizeof mh);
    mh.msg_iov = held ? iov : iov + 1;
    mh.msg_iovlen = held ? 2 : 1;
    ssize_t r;
    do r = recvmsg(ps.fd, &mh, MSG_PEEK | MSG_DONTWAIT);
    while (r < 0 && errno == EINTR);
    return r;
}

// Remove the socket's bytes up to stream position `to` (the owner holds a copy of them, read
// with MSG_PEEK).  TCP discards them without a copy (recv with MSG_TRUNC and no buffer); other
// stream sockets refuse that (EFAULT, nothing taken) and read into scratch.  `who` and `which`
// word the failure ("<who>: removing <which> bytes from socket ...").
inline int sock_consume(PeekSock& ps, uint64_t to, const char* who, const char* which) {
    while (ps.sock_pos < to) {
        const uint64_t want = to - ps.sock_pos;
        ssize_t r;
        if (ps.tcp) {
            r = recv(ps.fd, nullptr, (size_t)want, MSG_TRUNC | MSG_DONTWAIT);
            if (r < 0 && errno == EFAULT) {
                ps.tcp = 0;   // this socket copies: use the scratch from now on
                continue;
            }
        } else {
            if (!ps.scratch && !(ps.scratch = (uint8_t*)malloc(kDiscardBytes)))
                return netc_gpu::api_fail(NETC_GPU_ENOMEM, "%s: discard buffer", who);
            r = recv(ps.fd, ps.scratch, (size_t)(want < kDiscardBytes ? want : kDiscardBytes), MSG_DONTWAIT);
        }
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0)   // the bytes were peeked, so they are there: the socket has failed
            return recv_failed(r < 0 ? errno : ECONNRESET, "%s: removing %s bytes from socket %d", who, which, ps.fd);
        ps.sock_pos += (uint64_t)r;
    }
    return 0;
}

// ---------------------------------------------------------------- message reassembly --

// room for `need` bytes in a malloc'd buffer (doubling); false when out of memory.  A null
// buffer is allocated even for need 0, so an empty message still gets a buffer.
inline bool grow(uint8_t*& buf, size_t& cap, size_t need) {
    if (need <= cap && buf) return true;
    size_t c = cap ? cap : 256;
    while (c < need) c *= 2;
    uint8_t* nb = (uint8_t*)realloc(buf, c);
    if (!nb) return false;
    buf = nb;
    cap = c;
    return true;
}

// the reference's reassembly state, src/ws/common.c:163-164,210-216,303-309,333-347
struct MsgBuf {
    uint8_t* buf = nullptr;      // the message so far (malloc; the caller's once delivered)
    size_t size = 0, cap = 0;
    uint8_t opcode = 0;          // the last non-continuation frame's opcode, as the reference
};

inline bool msg_append(MsgBuf& m, const uint8_t* p, size_t n) {
    if (!grow(m.buf, m.cap, m.size + n)) return false;
    if (n) memcpy(m.buf + m.size, p, n);
    m.size += n;
    return true;
}

// One unmasked frame (header byte 0, payload) joins the message.  0: FIN completed it and *out
// is the message as ws_parse_frame fills it (a TEXT message has its NUL, an empty one still a
// buffer; the buffer is the caller's now); 1: more frames to come;
// WS_FRAME_PARSE_ERROR_PAYLOAD_TOO_BIG against the caller's limit; NETC_GPU_ENOMEM (no message
// set: the caller words it).
inline int msg_add_frame(MsgBuf& m, uint8_t b0, const uint8_t* payload, uint64_t len, size_t max_payload_length,
                         struct ws_message* out) {
    const uint8_t op = b0 & 0x0F;
    if (op != WS_OPCODE_CONTINUE) m.opcode = op;                                             // :163-164
    if (len + m.size > max_payload_length) return WS_FRAME_PARSE_ERROR_PAYLOAD_TOO_BIG;      // :210-211, :261-262
    if (!msg_append(m, payload, (size_t)len)) return NETC_GPU_ENOMEM;
    if (!(b0 & 0x80)) return 1;
    // FIN: the message (:340-346)
    if (m.opcode == WS_OPCODE_TEXT && !msg_append(m, (const uint8_t*)"", 1)) return NETC_GPU_ENOMEM;
    out->opcode = m.opcode;
    out->buffer = m.buf;
    out->payload_length = m.size;
    m.buf = nullptr;
    m.size = m.cap = 0;
    return 0;
}

}  // namespace
