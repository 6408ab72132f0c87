// Host-resident messages framed and masked on the GPU into a pinned ring, then sent on a socket:
// include/ws/egress.h (SURVEY.md §8(f) row 2 from a caller's host buffers).
//
// The reference frames a message per frame with three copies and a byte loop
// (ws_send_message, src/ws/common.c:96-119) and one send() per frame (:121).  Here a
// message is appended to a page-locked payload slot (the one host copy) while its frame
// table -- payload offsets, key32, header byte 0 per frame, the reference's split
// (:42-49) -- is written beside it.  Per submitted slot, on the slot's own HIP stream:
//
//   H2D     the payload bytes, then the packed table (offsets | keys | header bytes: one copy)
//   encode  launch_encode_frames (ws_frame_gpu.hip): wire offsets, then every frame's header,
//           key and masked payload back to back -- one launch when every frame of the slot is
//           in one length class (the host saw each length: the offsets are affine, no scan)
//   D2H     the wire bytes into the slot's page-locked wire buffer (the host knows their
//           count: it summed the header lengths while queueing) and the device's own wire
//           length beside them, checked against it when the slot is taken; event "done"
//
// Slots are independent (each frame's wire position depends only on its own slot), so the
// next slot fills while this one is on the GPU and an older one goes out on the socket.
//
// The slot itself -- its buffers, the frame split, the submission -- is ws_ring_host.h's
// SendSlot, shared with the egress hub (ws_egress_hub.hip); this file is the ring around it:
// the FIFO of submitted slots, the hand-out (next / release) and the one attached socket.
#include <hip/hip_runtime.h>

#include <errno.h>
#include <stdint.h>
#include <string.h>
#include <sys/uio.h>

#include <new>

#include "ws_ring_host.h"

extern "C" {
#include "../../include/ws/egress.h"
#include "../../include/ws/route.h"
}

using netc_gpu::api_fail;
using netc_gpu::api_fail_hip;

namespace {

constexpr int kBadSend = 9;   // netc's BADSEND reason (include/utils/error.h)

enum SlotState : int { kFree = 0, kFilling, kInflight, kTaken };

struct EgressSlot : SendSlot {   // the shared send-side slot (ws_ring_host.h)
    uint64_t messages = 0;
};

}  // namespace

struct netc_ws_egress {
    int device = 0;
    int flags = 0;
    int nslots = 0;
    SendLayout lay;
    EgressSlot* slots = nullptr;
    int cur = -1;          // slot being filled, -1 = none
    int next_fill = 0;     // the slot to fill next (ring order)
    int fifo[16] = {0};    // submitted slots not yet handed out, in queue order
    int head = 0, count = 0;
    int owner_fd = -1;     // the socket served through ws_send_message (netc_ws_gpu_attach_send)
    SockId owner_id;
};

namespace {

// Queue the filling slot on the GPU (see the file comment).
int submit_cur(netc_ws_egress* g) {
    if (g->cur < 0) return 0;
    EgressSlot& s = g->slots[g->cur];
    if (s.frames == 0) return 0;
    if (netc_gpu::inject_fault())
        return api_fail(NETC_GPU_ELAUNCH, "egress: injected fault (NETC_GPU_KNOB_INJECT_FAULT)");
    if (int r = send_slot_submit(g->lay, s, "egress")) return r;
    s.state = kInflight;
    g->fifo[(g->head + g->count) % 16] = g->cur;
    ++g->count;
    g->cur = -1;
    return 0;
}

// make a slot the filling one (ring order); NETC_WS_EGRESS_FULL if it is still in use
int acquire(netc_ws_egress* g) {
    if (g->cur >= 0) return 0;
    EgressSlot& s = g->slots[g->next_fill];
    if (s.state != kFree) return api_fail(NETC_WS_EGRESS_FULL, "egress: no free slot (send or release wire batches)");
    s.state = kFilling;
    s.masked = -1;
    s.fill = s.frames = s.messages = s.wire = 0;
    s.ext = -2;
    g->cur = g->next_fill;
    g->next_fill = (g->next_fill + 1) % g->nslots;
    return 0;
}

// [p, p + n) on fd without waiting for the peer: what the socket does not take joins the
// connection's send backlog (include/ws/route.h), ahead of its later bytes
int send_all(int fd, const uint8_t* p, uint64_t n) {
    struct iovec v = {(void*)p, (size_t)n};
    if (netc_ws_send_nb(fd, &v, 1, 1) == 1) return 0;
    const int saved = errno;
    api_fail(NETC_WS_EGRESS_ESEND, "egress: send: %s", strerror(saved));
    netc_errno_reason = kBadSend;
    errno = saved;
    return NETC_WS_EGRESS_ESEND;
}

}  // namespace

extern "C" {

int netc_ws_egress_create(struct netc_ws_egress** out, int device, size_t slot_bytes, int nslots, size_t max_frames,
                          int flags) {
    if (!out) return api_fail(NETC_GPU_EINVAL, "egress: null output pointer");
    *out = nullptr;
    if (int r = netc_gpu::api_check_device(device)) return r;
    if (flags & ~NETC_WS_EGRESS_DEFER) return api_fail(NETC_GPU_EINVAL, "egress: unknown flags 0x%x", flags);
    if (!slot_bytes) slot_bytes = 16u << 20;
    if (!nslots) nslots = 4;
    if (!max_frames) max_frames = slot_bytes / 64 + 64;
    if (slot_bytes < 4096 || slot_bytes > (1ull << 40) || nslots < 2 || nslots > 16 || max_frames > (1ull << 32))
        return api_fail(NETC_GPU_EINVAL, "egress: need 4096 <= slot_bytes <= 2^40, 2 <= nslots <= 16, "
                                         "max_frames <= 2^32");
    DeviceGuard dg(device);
    if (dg.err != hipSuccess) return api_fail_hip(NETC_GPU_ERUNTIME, "hipSetDevice", dg.err);
    netc_ws_egress* g = new (std::nothrow) netc_ws_egress();
    if (!g) return api_fail(NETC_GPU_ENOMEM, "egress: host allocation");
    g->device = device;
    g->flags = flags;
    g->nslots = nslots;
    g->lay = send_layout(slot_bytes, max_frames);
    g->slots = new (std::nothrow) EgressSlot[nslots];
    if (!g->slots) {
        delete g;
        return api_fail(NETC_GPU_ENOMEM, "egress: host allocation");
    }
    for (int i = 0; i < nslots; ++i) {
        if (int r = send_slot_alloc(g->lay, g->slots[i], "egress")) {
            for (int j = 0; j <= i; ++j) send_slot_free(device, g->slots[j]);
            delete[] g->slots;
            delete g;
            return r;
        }
    }
    *out = g;
    return 0;
}

void netc_ws_egress_destroy(struct netc_ws_egress* g) {
    if (!g) return;
    DeviceGuard dg(g->device);
    for (int i = 0; i < g->nslots; ++i) send_slot_free(g->device, g->slots[i]);
    delete[] g->slots;
    delete g;
}

int netc_ws_egress_queue(struct netc_ws_egress* g, const void* payload, size_t len, uint8_t opcode,
                         const uint8_t* masking_key, size_t num_frames) {
    if (!g || (len && !payload)) return api_fail(NETC_GPU_EINVAL, "egress: null argument");
    const uint64_t nf = num_frames ? num_frames : 1;
    const int masked = masking_key ? 1 : 0;
    const SendLayout& l = g->lay;
    if (len > l.slot_bytes || nf > l.max_frames)
        return api_fail(NETC_WS_EGRESS_TOO_BIG, "egress: a message of %zu bytes in %llu frames exceeds a slot "
                        "(%llu bytes, %llu frames)", len, (unsigned long long)nf,
                        (unsigned long long)l.slot_bytes, (unsigned long long)l.max_frames);
    if (int r = acquire(g)) return r;
    {
        const EgressSlot& s = g->slots[g->cur];
        if (s.frames && (s.masked != masked || s.fill + len > l.slot_bytes || s.frames + nf > l.max_frames)) {
            DeviceGuard dg(g->device);   // (only here: a HIP call per queued message costs ~15 % at 1 KiB)
            if (dg.err != hipSuccess) return api_fail_hip(NETC_GPU_ERUNTIME, "hipSetDevice", dg.err);
            if (int e = submit_cur(g)) return e;
            if (int r = acquire(g)) return r;
        }
    }
    EgressSlot& s = g->slots[g->cur];
    (void)send_slot_append(s, l, payload, len, opcode, masking_key, nf);
    ++s.messages;
    return 0;
}

int netc_ws_egress_submit(struct netc_ws_egress* g) {
    if (!g) return api_fail(NETC_GPU_EINVAL, "egress: null egress");
    DeviceGuard dg(g->device);
    if (dg.err != hipSuccess) return api_fail_hip(NETC_GPU_ERUNTIME, "hipSetDevice", dg.err);
    return submit_cur(g);
}

int netc_ws_egress_next(struct netc_ws_egress* g, struct netc_ws_wire* out, int wait) {
    if (!g || !out) return api_fail(NETC_GPU_EINVAL, "egress: null argument");
    if (g->count == 0) return 0;
    DeviceGuard dg(g->device);
    if (dg.err != hipSuccess) return api_fail_hip(NETC_GPU_ERUNTIME, "hipSetDevice", dg.err);
    const int i = g->fifo[g->head];
    EgressSlot& s = g->slots[i];
    hipError_t e = wait ? hipEventSynchronize(s.done) : hipEventQuery(s.done);
    if (!wait && e == hipErrorNotReady) return 0;
    if (e != hipSuccess) return api_fail_hip(NETC_GPU_ERUNTIME, "egress: slot wait", e);
    g->head = (g->head + 1) % 16;
    --g->count;
    if (*s.h_len != s.wire) {   // the device's wire length against the host's header sum
        s.state = kFree;
        return api_fail(NETC_GPU_ERUNTIME, "egress: device wire length %llu, expected %llu",
                        (unsigned long long)*s.h_len, (unsigned long long)s.wire);
    }
    out->wire = s.h_wire;
    out->len = s.wire;
    out->nframes = s.frames;
    out->nmessages = s.messages;
    out->slot = i;
    s.state = kTaken;
    return 1;
}

int netc_ws_egress_release(struct netc_ws_egress* g, const struct netc_ws_wire* w) {
    if (!g || !w || w->slot < 0 || w->slot >= g->nslots || g->slots[w->slot].state != kTaken)
        return api_fail(NETC_GPU_EINVAL, "egress: not a wire batch handed out by this egress");
    g->slots[w->slot].state = kFree;
    return 0;
}

long netc_ws_egress_send(struct netc_ws_egress* g, int fd, int wait) {
    if (!g) return api_fail(NETC_GPU_EINVAL, "egress: null egress");
    long total = 0;
    for (;;) {
        struct netc_ws_wire w;
        const int r = netc_ws_egress_next(g, &w, wait);
        if (r < 0) return r;
        if (r == 0) return total;
        const int s = send_all(fd, w.wire, w.len);
        (void)netc_ws_egress_release(g, &w);
        if (s) return s;
        total += (long)w.len;
    }
}

long netc_ws_egress_flush(struct netc_ws_egress* g, int fd) {
    if (int r = netc_ws_egress_submit(g)) return r;
    return netc_ws_egress_send(g, fd, 1);
}

// ws_send_message on a socket attached to a ring (include/ws/route.h): the reference's send
// contract (src/ws/common.c:36-130: 1 once sent, else the failing send() result) served from
// the ring.  DEFER rings return once the message is queued and send what has finished.
static int gpu_send_route(void* ctx, int sockfd, struct ws_message* message, uint8_t masking_key[4],
                          size_t num_frames) {
    netc_ws_egress* g = (netc_ws_egress*)ctx;
    if (sockfd != g->owner_fd) {   // one ring, one connection: never another socket's bytes
        api_fail(NETC_GPU_EINVAL, "send route: the ring serves socket %d, not %d", g->owner_fd, sockfd);
        return -1;
    }
    int r = netc_ws_egress_queue(g, message->buffer, message->payload_length, message->opcode, masking_key,
                                 num_frames);
    if (r == NETC_WS_EGRESS_FULL) {   // every slot queued or unsent: put the oldest on the socket
        if (netc_ws_egress_send(g, sockfd, 1) < 0) return -1;
        r = netc_ws_egress_queue(g, message->buffer, message->payload_length, message->opcode, masking_key,
                                 num_frames);
    }
    if (r) return -1;
    // a DEFER ring sends what has finished; a close frame goes out at once, with everything
    // queued before it (netc closes the socket right after sending one, src/ws/server.c:123-124)
    const bool now = !(g->flags & NETC_WS_EGRESS_DEFER) || message->opcode == WS_OPCODE_CLOSE;
    const long s = now ? netc_ws_egress_flush(g, sockfd) : netc_ws_egress_send(g, sockfd, 0);
    return s < 0 ? -1 : 1;
}

// close() on the attached socket (close tracking, include/ws/route.h): what it queued goes out first
static void ring_close_hook(void* ctx, int sockfd) { (void)netc_ws_gpu_detach_send(sockfd); }

// a ring's messages queued but not yet on its socket (slots filling, on the GPU or finished)
static bool has_queued(const netc_ws_egress* g) {
    return g->count > 0 || (g->cur >= 0 && g->slots[g->cur].frames > 0);
}

int netc_ws_gpu_attach_send(int sockfd, struct netc_ws_egress* ring) {
    if (!ring) return api_fail(NETC_GPU_EINVAL, "attach_send: null ring");
    SockId id;
    if (!sock_identity(sockfd, &id))
        return api_fail(NETC_GPU_EINVAL, "attach_send: %d is not an open socket", sockfd);
    if (ring->owner_fd >= 0) {
        if (ring->owner_fd == sockfd && ring->owner_id == id) return 0;
        if (same_socket(ring->owner_fd, ring->owner_id))
            return api_fail(NETC_GPU_EINVAL, "attach_send: the ring already serves socket %d (one ring, one "
                            "connection)", ring->owner_fd);
        // its connection was closed without a detach
        void* ctx = nullptr;
        if (netc_ws_send_route_get_raw(ring->owner_fd, &ctx) && ctx == ring) (void)netc_ws_send_route_detach(ring->owner_fd);
        ring->owner_fd = -1;
    }
    if (has_queued(ring))   // they were queued for another connection
        return api_fail(NETC_GPU_EINVAL, "attach_send: the ring holds queued messages (flush or destroy it first)");
    if (netc_ws_send_route_attach(sockfd, gpu_send_route, ring) != 0)
        return api_fail(NETC_GPU_EINVAL, "attach_send: socket %d: %s", sockfd,
                        errno == EBUSY ? "another send route serves it" : "out of range");
    ring->owner_fd = sockfd;
    ring->owner_id = id;
    (void)netc_ws_send_route_on_close(sockfd, ring_close_hook);
    return 0;
}

int netc_ws_gpu_detach_send(int sockfd) {
    if (sockfd < 0) return api_fail(NETC_GPU_EINVAL, "detach_send: socket %d out of range", sockfd);
    void* ctx = nullptr;
    long flushed = 0;
    if (netc_ws_send_route_get_raw(sockfd, &ctx) == gpu_send_route && ctx) {
        netc_ws_egress* g = (netc_ws_egress*)ctx;
        if (g->owner_fd == sockfd) {
            // ws_send_message already returned 1 for a DEFER ring's queued messages: they go out now
            if (has_queued(g)) {
                if (same_socket(sockfd, g->owner_id))
                    flushed = netc_ws_egress_flush(g, sockfd);
                else
                    flushed = api_fail(NETC_WS_EGRESS_ESEND, "detach_send: socket %d was closed with queued "
                                       "messages", sockfd);
            }
            g->owner_fd = -1;
        }
    }
    if (netc_ws_send_route_detach(sockfd) != 0)
        return api_fail(NETC_GPU_EINVAL, "detach_send: socket %d out of range", sockfd);
    return flushed < 0 ? (int)flushed : 0;
}

}  // extern "C"
