// lexeme_input.h -- what the two lexeme entry points (resolve.hip: queries; cast.hip: documents) share on the host: the seed as the
// words intern_lane takes, the limit of the chaining-value stack, and the validation of a packed lexeme pool with its refusal texts.
#ifndef VBM25_LEXEME_INPUT_H
#define VBM25_LEXEME_INPUT_H

#include <algorithm>
#include <cstdint>
#include <cstring>

#include "vbm25_internal.h"
#include "resolve_lane.h"

namespace vbm25 {
namespace lexin {

constexpr uint32_t MAX_LEVELS = 32;  // 64 KiB of LDS at one wave a block: lexemes up to 2^32 chunks
constexpr const char *NEEDS_SEED = "a lexeme of 16 bytes or more needs the index's seed (Meta tuple)";

struct Seed {
    uint32_t w[8];
};
inline void seed_words(const uint8_t *seed32, Seed *s) {
    for (int i = 0; i < 8; ++i)
        s->w[i] = seed32 ? uint32_t(seed32[4 * i]) | uint32_t(seed32[4 * i + 1]) << 8 | uint32_t(seed32[4 * i + 2]) << 16 | uint32_t(seed32[4 * i + 3]) << 24 : 0u;
}

// n_lex lexemes, lexeme i = bytes[lex_off[i] .. lex_off[i + 1]): monotone offsets, bytes present, no lexeme over the stack's limit
// (`who`: "resolver" / "cast"), and -- without a seed -- none that needs the hash.  Fills the pool's length and the longest lexeme.
inline int check_pool(bool has_seed, const uint8_t *bytes, const uint64_t *lex_off, uint32_t n_lex, const char *who, uint64_t *n_bytes,
                      uint64_t *longest_lexeme) {
    bool hashed = false;
    for (uint32_t i = 0; i < n_lex; ++i) {
        if (lex_off[i + 1] < lex_off[i]) return set_error(VBM25_ERR_INVALID, "lex_off is not monotone at lexeme %u", i);
        const uint64_t len = lex_off[i + 1] - lex_off[i];
        *longest_lexeme = std::max(*longest_lexeme, len);
        hashed |= len >= 16;
    }
    *n_bytes = lex_off[n_lex];
    if (*n_bytes && !bytes) return set_error(VBM25_ERR_INVALID, "NULL argument");
    if (rsv::stack_levels(*longest_lexeme) > MAX_LEVELS)
        return set_error(VBM25_ERR_INVALID, "a lexeme of %llu bytes is over the %s's limit", (unsigned long long)*longest_lexeme, who);
    if (!has_seed) {  // (every lexeme is short here or refused: a NUL anywhere in the lexemes' bytes is a NUL inside one of them)
        if (hashed || (*n_bytes > lex_off[0] && std::memchr(bytes + lex_off[0], 0, *n_bytes - lex_off[0])))
            return set_error(VBM25_ERR_INVALID, "%s", NEEDS_SEED);
    }
    return VBM25_OK;
}

}  // namespace lexin
}  // namespace vbm25

#endif
