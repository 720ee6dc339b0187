// vv_ckpt_format.hpp -- the checkpoint blob's format as host code without any HIP dependency (include/vvhip.h: "checkpoint"): the digest,
// the layout of header / table / payloads and the parser.  vv_checkpoint.cpp builds blobs with it; tests build it alone with g++.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/vvhip.h"

#pragma GCC visibility push(hidden)
namespace vvckpt {

constexpr size_t kHeaderDigested = offsetof(vvhip_checkpoint_header, header_digest);      // bytes of the header its digest covers
inline size_t align16(size_t x) { return (x + 15) & ~(size_t) 15; }
const char* section_name(uint32_t id);
// the digest of `bytes` (a multiple of 4) at any alignment
uint64_t digest(const void* data, size_t bytes, uint64_t base);
uint64_t header_digest(const vvhip_checkpoint_header& h, const vvhip_checkpoint_section* table);
// Every check of vvhip_checkpoint_inspect.  hdr / table (VVHIP_CKPT_SECTIONS entries) receive copies: the blob may sit at any alignment.
int inspect(const void* blob, size_t bytes, vvhip_checkpoint_header* hdr, vvhip_checkpoint_section* table, std::string& err);

}  // namespace vvckpt
#pragma GCC visibility pop
