// The digit functions of csrc/key_tables.h and csrc/verify_core.h (kt_digit, comb_digit) from both of their sources -- the
// registers of a lane and a [word][lane] array as key_verify_kernel keeps it in LDS -- beside the extraction as it stood
// in line in kt_add_digit and add_comb_range before it became a function, kept here word for word; and the first addition
// of a sum in both forms (kt_first_entry, kt_add_entry from the identity).  A library for tests/test_key_digits_host.py,
// which holds every output against the textbook digits and the Python oracle's points.  It only executes.
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "../../jubjub_schnorr_amd/tools/scalar_stages.h"

using namespace jjs;

namespace {

constexpr int LANES = 64;

// kt_add_digit's digit as it was written in line: the signed digit whose magnitude is the entry that was loaded
int digit_in_line(const words8& sc, int pos, int w) {
    const int bit = w * pos, wi = bit >> 5, sh = bit & 31;
    uint32_t v = word_at(sc, wi) >> sh;
    if (sh + w > 32) v |= word_at(sc, wi + 1 > 7 ? 7 : wi + 1) << (32 - sh);
    const uint32_t raw = v & ((1u << w) - 1u);
    const bool top = pos == kt_positions(w) - 1;
    const int d = top ? (int)(word_at(sc, wi) >> sh) : (int)raw - (1 << (w - 1));
    const bool neg = d < 0;
    uint32_t idx = (uint32_t)(neg ? -d : d);
    idx = idx >= (uint32_t)kt_entries(w) ? (uint32_t)kt_entries(w) - 1u : idx;
    return neg ? -(int)idx : (int)idx;
}
// add_comb_range's digit as it was written in line
uint32_t comb_digit_in_line(const words8& k, int i) {
    constexpr int per_word = 32 / COMB_BITS;
    return (word_at(k, i / per_word) >> ((i % per_word) * COMB_BITS)) & (uint32_t)(COMB_ENTRIES - 1);
}

int as_int(const kt_signed_digit& d) { return d.neg ? -(int)d.idx : (int)d.idx; }

}  // namespace

extern "C" {

int jjs_kd_positions(int w) { return kt_positions(w); }
int jjs_kd_comb_windows() { return COMB_WINDOWS; }

// s: n scalars of 8 words.  Per scalar and position: the digit from the registers, from the lanes array (the scalars of a
// group of 64 lie side by side in it, each lane reads its own column) and in line -> n x positions each; the same for the
// comb's digits of the scalar as it is -> n x COMB_WINDOWS each.
int jjs_kd_digits(const uint32_t* s, size_t n, int w, int32_t* regs, int32_t* lanes, int32_t* in_line, uint32_t* comb_regs,
                  uint32_t* comb_lanes, uint32_t* comb_in_line) {
    if (w != KT_WINDOW_NARROW && w != KT_WINDOW_WIDE) return 1;
    const int positions = kt_positions(w);
    static uint32_t recoded[8][LANES], plain[8][LANES];
    for (size_t first = 0; first < n; first += LANES) {
        const size_t group = n - first < (size_t)LANES ? n - first : (size_t)LANES;
        memset(recoded, 0xA5, sizeof recoded);
        memset(plain, 0x5A, sizeof plain);
        for (size_t l = 0; l < group; ++l) {
            const words8 k = sc::ld8(s + 8 * (first + l));
            words_in_lanes<LANES>{&recoded[0][l]}.put(kt_recode(k, w));
            words_in_lanes<LANES>{&plain[0][l]}.put(k);
        }
        for (size_t l = 0; l < group; ++l) {
            const size_t i = first + l;
            const words8 k = sc::ld8(s + 8 * i), r = kt_recode(k, w);
            for (int pos = 0; pos < positions; ++pos) {
                regs[i * positions + pos] = as_int(kt_digit(words_in_regs{r}, pos, w));
                lanes[i * positions + pos] = as_int(kt_digit(words_in_lanes<LANES>{&recoded[0][l]}, pos, w));
                in_line[i * positions + pos] = digit_in_line(r, pos, w);
            }
            for (int j = 0; j < COMB_WINDOWS; ++j) {
                comb_regs[i * COMB_WINDOWS + j] = comb_digit(words_in_regs{k}, j);
                comb_lanes[i * COMB_WINDOWS + j] = comb_digit(words_in_lanes<LANES>{&plain[0][l]}, j);
                comb_in_line[i * COMB_WINDOWS + j] = comb_digit_in_line(k, j);
            }
        }
    }
    return 0;
}

// pt: the affine base (u, v: 16 words).  For d = -2^(w-1) .. 2^(w-1), in this order: kt_first_entry(table, d) and
// kt_add_entry(identity, table, d) as extended points of 36 words.
int jjs_kd_first_entry(const uint32_t* pt, int w, uint32_t* first, uint32_t* added) {
    if (w != KT_WINDOW_NARROW && w != KT_WINDOW_WIDE) return 1;
    uint32_t* tab = (uint32_t*)aligned_alloc(16, (size_t)kt_table_words(w) * 4);
    if (!tab) return 2;
    kt_build_table(tab, ext_from_affine(fq_from_words(sc::ld8(pt)), fq_from_words(sc::ld8(pt + 8))), kt_entries(w));
    const int last = kt_entries(w) - 1;
    for (int d = -last; d <= last; ++d) {
        const kt_signed_digit e{(uint32_t)(d < 0 ? -d : d), d < 0};
        sc::st_pt(first + 36 * (d + last), kt_first_entry(tab, e));
        sc::st_pt(added + 36 * (d + last), kt_add_entry(ext_identity(), tab, e));
    }
    free(tab);
    return 0;
}

}  // extern "C"
