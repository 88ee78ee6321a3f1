// Stand-alone CPU check of the canonical orientation's definition in csrc/nn/symmetry.h (built with
// -fsanitize=address,undefined by tests/test_symmetry_canon.py): gzsym::canon_element, the serial
// statement the kernel follows, against a brute-force restatement -- materialise every image, tag it
// with gzcache::row_tag, rank by mix64(tag ^ salt), take the first minimum.  It prints what it computed,
//   canon E=<E> S=<S> salt=<salt> kind=<kind> g=<g> tag=<tag>
// and the test recomputes every line with numpy (util/symmetry.py canonical_elements).  The tables are
// the rotations plane_src[s][i] = (i + 3 s) mod E; kind "one" is its own image under every element and
// "period15" (1.0 where i mod 15 < 7) under the rotation by 15 where 15 divides E: ties go to the lowest s.
#include "../galvanise_zero_amd/csrc/nn/eval_cache.h"

#include <cassert>
#include <cstring>

using namespace gzsym;

static void make_row(const char* kind, int E, unsigned* bits) {
    for (int i = 0; i < E; ++i) bits[i] = 0u;
    if (!strcmp(kind, "one")) for (int i = 0; i < E; ++i) bits[i] = 0x3F800000u;
    if (!strcmp(kind, "negzero")) bits[E / 2] = 0x80000000u;
    if (!strcmp(kind, "nan")) bits[E - 1] = 0x7FC00123u;
    if (!strcmp(kind, "period15")) for (int i = 0; i < E; ++i) bits[i] = i % 15 < 7 ? 0x3F800000u : 0u;
    if (!strcmp(kind, "lcg")) {
        unsigned x = 12345u + (unsigned)E;
        for (int i = 0; i < E; ++i) {
            x = x * 1664525u + 1013904223u;
            bits[i] = ((x >> 16) & 1u) ? 0x3F800000u : 0u;
        }
    }
}

static int brute(const unsigned* bits, int E, int S, const int* plane_src, unsigned salt, unsigned long long* tag,
                 std::vector<std::vector<unsigned>>* images) {
    images->assign((size_t)S, std::vector<unsigned>((size_t)E));
    int g = -1;
    unsigned long long best = 0;
    for (int s = 0; s < S; ++s) {
        std::vector<unsigned>& im = (*images)[(size_t)s];
        for (int i = 0; i < E; ++i) im[(size_t)i] = bits[plane_src[(size_t)s * E + i]];
        const unsigned long long t = gzcache::row_tag(im.data(), E), k = gzcache::mix64(t ^ (unsigned long long)salt);
        if (g < 0 || k < best) { g = s; best = k; *tag = t; }
    }
    return g;
}

int main() {
    const int Es[] = {75, 320, 1300};
    const int Ss[] = {1, 2, 3, 8};
    const unsigned salts[] = {0u, 0xFFFFFFFFu};
    const char* kinds[] = {"lcg", "one", "negzero", "nan", "period15"};
    int ties = 0, moved = 0;
    for (int E : Es)
        for (int S : Ss) {
            std::vector<int> plane((size_t)S * E);
            for (int s = 0; s < S; ++s)
                for (int i = 0; i < E; ++i) plane[(size_t)s * E + i] = (i + 3 * s) % E;
            int bad = 0;
            for (int s = 0; s < S; ++s) assert(is_permutation(plane.data() + (size_t)s * E, E, &bad));
            std::vector<unsigned> bits((size_t)E);
            for (const char* kind : kinds) {
                make_row(kind, E, bits.data());
                int g_salt[2];
                for (int k = 0; k < 2; ++k) {
                    unsigned long long tag = 0, ref_tag = 0;
                    std::vector<std::vector<unsigned>> images;
                    const int g = canon_element(bits.data(), E, S, plane.data(), salts[k], &tag);
                    const int ref = brute(bits.data(), E, S, plane.data(), salts[k], &ref_tag, &images);
                    assert(g == ref && tag == ref_tag && g >= 0 && g < S);
                    assert(canon_element(bits.data(), E, S, plane.data(), salts[k], nullptr) == g);
                    // of equal images the lowest s is taken
                    for (int s = 0; s < g; ++s) assert(images[(size_t)s] != images[(size_t)g]);
                    for (int s = g + 1; s < S; ++s) ties += images[(size_t)s] == images[(size_t)g];
                    if (!strcmp(kind, "one")) assert(g == 0);
                    if (!strcmp(kind, "period15") && E % 15 == 0) assert(g < 5);   // the rotation by 15 is s = 5
                    g_salt[k] = g;
                    printf("canon E=%d S=%d salt=%u kind=%s g=%d tag=%llu\n", E, S, salts[k], kind, g, tag);
                }
                moved += g_salt[0] != g_salt[1];
            }
        }
    assert(ties > 0);                            // rows equal to one of their images were met
    assert(moved > 0);                           // another salt, another representative
    printf("symmetry canon host check passed\n");
    return 0;
}
