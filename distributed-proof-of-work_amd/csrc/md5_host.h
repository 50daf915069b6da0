// md5_host.h -- host MD5 used by the planner (midstates) and hit verification.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/dpow.h"

namespace dpow {
void md5_compress(uint32_t st[4], const uint32_t M[16]);
void md5_digest(const uint8_t *msg, size_t len, uint8_t out[16]);
uint32_t digest_trailing_zero_nibbles(const uint8_t d[16]);
uint32_t load_le32(const uint8_t *p);
// The depth (trailing '0' characters of the MD5) of nonce || secret of global index g.  msg holds
// the nonce (nonce_len bytes) in front of DPOW_MAX_SECRET free bytes, which receive the secret;
// the digest goes to `digest` and the secret's length to `secret_len` where they are not null.
uint32_t md5_depth_of_index(uint8_t *msg, size_t nonce_len, uint64_t g, uint8_t *digest = nullptr,
                            size_t *secret_len = nullptr);
// `msg` as md5_depth_of_index takes it, for this nonce: resized, the nonce copied to its front.
__attribute__((visibility("hidden"))) inline uint8_t *md5_msg_of_nonce(std::vector<uint8_t> &msg, const uint8_t *nonce,
                                                                       size_t nonce_len) {
    msg.resize(nonce_len + DPOW_MAX_SECRET);
    if (nonce_len) memcpy(msg.data(), nonce, nonce_len);
    return msg.data();
}
}  // namespace dpow
