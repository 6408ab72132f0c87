// Internal interface between the frame decode (ws_decode_gpu.hip) and the C-ABI layer
// (ws_mask_api.hip).  Not installed; the public surface is include/ws/frame.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace netc_gpu {

// ws_decode_gpu.hip: the frames a scan recorded (hdr / keys / b0 / max_frames / result, read
// on the device) as a mask.h batch -- payloads unmasked back to back into payload, n + 1
// offsets, the message table (msg_first / msg_opcode: both set or both null) and dresult.
// len > 0 and payload does not overlap wire.  Scratch (two status words per scan tile) is kept
// per (device, stream) until release_dec_scratch.
hipError_t launch_decode_frames(uint8_t* payload, uint64_t* offsets, uint64_t* msg_first, uint8_t* msg_opcode,
                                uint64_t* dresult, const uint8_t* wire, uint64_t len, const uint64_t* hdr,
                                const uint32_t* keys, const uint8_t* b0, uint64_t max_frames, const uint64_t* result,
                                hipStream_t stream);
int release_dec_scratch(int device, hipStream_t stream);   // 1 if there was a cached entry; the stream is synchronised

}  // namespace netc_gpu
