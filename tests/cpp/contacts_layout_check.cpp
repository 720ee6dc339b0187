// Host check of vv::contacts_layout and the two work-list builders (csrc/vv_layout.h), a program of its own: built with
// -fsanitize=address,undefined by tests/test_contacts.py.  Two classes (a x b, b x a) for every pair of site counts out of 0, 1, 63, 64, 65,
// 4097, under a few (num_lags, origin_every, continuous, rows per tile, words per item).  The lists are built into arrays of exactly the
// counted size, and every word of a matrix must be covered exactly once by the mask items (64 rows x 1 column word at a time, as the
// kernel stores them) and by the correlate items (two words at a time), with one designated item per class.  Prints one line per case for
// the test to hold against tests/contacts_reference.py: layout(); exit status 1 and a message where a list is wrong.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "vv_layout.h"

static int fail(const char* what, int na, int nb) {
    std::printf("FAIL %s at %d x %d\n", what, na, nb);
    return 1;
}

int main() {
    const int counts[6] = {0, 1, 63, 64, 65, 4097};
    struct Shape { int lags, every, continuous, tile, run; };
    const Shape shapes[3] = {{5, 2, 1, 128, 4}, {1, 1, 0, 64, 1}, {4096, 4, 1, 1024, 64}};
    for (const Shape& sh : shapes)
        for (int na : counts)
            for (int nb : counts) {
                const int rows[2] = {na, nb}, cols[2] = {nb, na};
                const vv::ContactsLayout L = vv::contacts_layout(2, rows, cols, sh.lags, sh.every, sh.continuous != 0, (long long) na + nb, 4);
                const long long nm = vv::contacts_mask_items(L, 2, sh.tile, sh.run, nullptr);
                const long long nc = vv::contacts_corr_items(L, 2, nullptr);
                vv::ContactsMaskItem* mi = new vv::ContactsMaskItem[nm > 0 ? nm : 1];
                vv::ContactsCorrItem* ci = new vv::ContactsCorrItem[nc];
                if (vv::contacts_mask_items(L, 2, sh.tile, sh.run, mi) != nm || vv::contacts_corr_items(L, 2, ci) != nc) return fail("count", na, nb);
                std::vector<unsigned char> seen((size_t) L.sample_words, 0);
                for (long long k = 0; k < nm; k++) {
                    const vv::ContactsMaskItem& it = mi[k];
                    if (it.cls < 0 || it.cls > 1 || it.i0 % 64 || it.i1 % 64 || it.i0 >= it.i1 || it.i1 - it.i0 > sh.tile || it.i1 > L.rows_padded[it.cls] ||
                        it.jw0 >= it.jw1 || it.jw1 - it.jw0 > sh.run || it.jw1 > L.col_words[it.cls])
                        return fail("mask item", na, nb);
                    for (int jw = it.jw0; jw < it.jw1; jw++)
                        for (int i = it.i0; i < it.i1; i++) {
                            const long long at = L.class_offset[it.cls] + (long long) jw * L.rows_padded[it.cls] + i;
                            if (at < 0 || at >= L.sample_words || seen[(size_t) at]++) return fail("mask cover", na, nb);
                        }
                }
                for (unsigned char s : seen) if (s != 1) return fail("mask gap", na, nb);
                int firsts[2] = {0, 0};
                std::vector<unsigned char> pair((size_t) (L.sample_words / 2), 0);
                for (long long k = 0; k < nc; k++) {
                    const vv::ContactsCorrItem& it = ci[k];
                    if (it.cls < 0 || it.cls > 1 || it.np < 0 || it.np > vv::CONTACTS_CORR_PAIRS) return fail("corr item", na, nb);
                    firsts[it.cls] += it.first != 0;
                    for (int q = 0; q < it.np; q++) {
                        const long long p = it.p0 + q;
                        if (2 * p < L.class_offset[it.cls] || 2 * p + 1 >= L.class_offset[it.cls] + L.class_words[it.cls] || pair[(size_t) p]++) return fail("corr cover", na, nb);
                    }
                }
                for (unsigned char s : pair) if (s != 1) return fail("corr gap", na, nb);
                if (firsts[0] != 1 || firsts[1] != 1 || L.sample_words % 64 || L.class_offset[1] % 2) return fail("designated item", na, nb);
                std::printf("%d %d %d %d %d %d %d  %lld %lld %lld %lld %d %d %lld %lld %lld %lld %lld  %lld %lld\n", na, nb, sh.lags, sh.every, sh.continuous, sh.tile, sh.run,
                            L.rows_padded[0], L.col_words[0], L.class_words[1], L.sample_words, L.num_origins, L.ord_words, L.table_words, L.ring_words,
                            L.words_bytes, L.scratch_bytes, L.total_bytes, nm, nc);
                delete[] mi;
                delete[] ci;
            }
    return 0;
}
