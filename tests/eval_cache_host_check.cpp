// Stand-alone CPU check of the evaluation cache's definition in csrc/nn/eval_cache.h (built with
// -fsanitize=address,undefined by tests/test_eval_cache.py): the two row hashes, the tag and the slot,
// and the serial model of the table over scripted sequences of calls.  It prints what it computed --
//   hash E=<E> kind=<kind> h1=<h1> h2=<h2> tag=<tag>
//   slot E=<E> kind=<kind> N=<N> slot=<slot>
//   scn <name> N=<N> E=<E> bits=<tag bits> chunk=<chunk rows>
//   call <name> rows=<seed/word/kind,...> hits=<0|1 per row> digest=<d> inserts=<i> replaced=<r>
//   flush <name>
// -- and the test recomputes every line with numpy (util/evalcache.py), so the two statements of the
// definition are held to each other exactly.  A row of a call is lcg_row(seed) with one word changed:
// kind n (nothing), f (0.0 <-> 1.0), c (0.0), z (-0.0).
#include "../galvanise_zero_amd/csrc/nn/eval_cache.h"

#include <cassert>
#include <cstring>
#include <string>

using namespace gzcache;

static void lcg_row(unsigned seed, int E, unsigned* bits) {
    unsigned x = seed;
    for (int i = 0; i < E; ++i) {
        x = x * 1664525u + 1013904223u;
        bits[i] = ((x >> 16) & 1u) ? 0x3F800000u : 0u;
    }
}

static void make_row(const char* kind, int E, unsigned* bits) {
    for (int i = 0; i < E; ++i) bits[i] = 0u;
    if (!strcmp(kind, "one")) for (int i = 0; i < E; ++i) bits[i] = 0x3F800000u;
    if (!strcmp(kind, "negzero")) bits[0] = 0x80000000u;
    if (!strcmp(kind, "nan")) bits[E - 1] = 0x7FC00123u;
    if (!strcmp(kind, "lcg")) lcg_row(12345u + (unsigned)E, E, bits);
}

// both hashes in another order (a 4-lane strided tree from the end): the sums are modular
static unsigned long long tag_reordered(const unsigned* bits, int E) {
    unsigned a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0};
    for (int i = E - 1; i >= 0; --i) {
        a[i & 3] += gzsym::pick_term(bits[i], (unsigned)i);
        b[i & 3] += hash2_term(bits[i], (unsigned)i);
    }
    return make_tag((a[3] + a[1]) + (a[2] + a[0]), (b[3] + b[1]) + (b[2] + b[0]));
}

static void check_hashes() {
    const int Es[] = {1, 3, 75, 320, 5415};
    const char* kinds[] = {"zero", "one", "negzero", "nan", "lcg"};
    const unsigned long long Ns[] = {1, 2, 3, 64, 65536};
    for (int E : Es) {
        std::vector<unsigned> bits((size_t)E);
        unsigned long long t_zero = 0;
        for (const char* kind : kinds) {
            make_row(kind, E, bits.data());
            const unsigned long long tag = row_tag(bits.data(), E);
            assert(tag == tag_reordered(bits.data(), E));
            if (!strcmp(kind, "zero")) t_zero = tag;
            if (!strcmp(kind, "negzero")) assert(tag != t_zero);   // the key reads bit patterns
            printf("hash E=%d kind=%s h1=%u h2=%u tag=%llu\n", E, kind, gzsym::pick_hash(bits.data(), E), hash2(bits.data(), E), tag);
            for (unsigned long long N : Ns) {
                const unsigned long long s = slot_of(tag, N);
                assert(s < N);
                printf("slot E=%d kind=%s N=%llu slot=%llu\n", E, kind, N, s);
            }
        }
    }
    assert(tag_mask(0) == 0 && tag_mask(64) == ~0ull && tag_mask(1) == 1ull && tag_mask(63) == (~0ull >> 1));
    assert(claim_word(2, 0) > claim_word(1, 0) && claim_word(1, 0) > claim_word(1, 1) && claim_word(2, 2047) > claim_word(1, 0));
    assert(entry_out_off(75) == 80 && entry_words(75, 60) == 140 && entry_words(320, 313) % 4 == 0);
    assert(tag_bits(0, false) == 64 && tag_bits(0, true) == 0 && tag_bits(99, true) == 64 && tag_bits(-3, true) == 0);
    assert(chunk_rows(0) == kMaxChunkRows && chunk_rows(2) == 2 && chunk_rows(1 << 20) == kMaxChunkRows);
}

struct Row { unsigned seed; int word; char kind; };

static void build_row(const Row& r, int E, unsigned* bits) {
    lcg_row(r.seed, E, bits);
    assert(r.word >= 0 && r.word < E);
    if (r.kind == 'f') bits[r.word] = bits[r.word] ? 0u : 0x3F800000u;
    if (r.kind == 'c') bits[r.word] = 0u;
    if (r.kind == 'z') bits[r.word] = 0x80000000u;
}

struct Scenario {
    Model m;
    std::string name;
    Scenario(const char* name_, unsigned long long N, int E, int bits, int chunk) : m(N, E, bits, chunk), name(name_) {
        printf("scn %s N=%llu E=%d bits=%d chunk=%d\n", name_, N, E, bits, m.chunk);
    }
    std::string call(const std::vector<Row>& rows) {
        std::vector<unsigned> X(rows.size() * (size_t)m.E);
        std::string spec;
        for (size_t r = 0; r < rows.size(); ++r) {
            build_row(rows[r], m.E, X.data() + r * (size_t)m.E);
            spec += (r ? "," : "") + std::to_string(rows[r].seed) + "/" + std::to_string(rows[r].word) + "/" + rows[r].kind;
        }
        const long before = m.hits + m.forward_rows;
        const std::vector<int> hit = m.call(X.data(), (int)rows.size());
        assert(m.hits + m.forward_rows == before + (long)rows.size());
        std::string h;
        for (int v : hit) h += v ? '1' : '0';
        printf("call %s rows=%s hits=%s digest=%llu inserts=%ld replaced=%ld\n", name.c_str(), spec.c_str(), h.c_str(), m.digest(),
               m.inserts, m.replaced);
        return h;
    }
    void flush() {
        m.flush();
        printf("flush %s\n", name.c_str());
    }
};

static std::vector<Row> seeds(std::initializer_list<unsigned> s) {
    std::vector<Row> out;
    for (unsigned v : s) out.push_back(Row{v, 0, 'n'});
    return out;
}

static void check_model() {
    {   // a repeat of a call: all hits when N is large
        Scenario s("repeat", 65536, 75, 64, 0);
        assert(s.call(seeds({1, 2, 3, 4, 5})) == "00000");
        assert(s.call(seeds({1, 2, 3, 4, 5})) == "11111");
        assert(s.call(seeds({5, 6, 1, 7})) == "1010");
        assert(s.m.inserts == 7 && s.m.replaced == 0);
    }
    {   // N = 1: only the newest key survives
        Scenario s("n1", 1, 75, 64, 0);
        assert(s.call(seeds({1})) == "0");
        assert(s.call(seeds({2})) == "0");
        assert(s.call(seeds({1})) == "0");
        assert(s.call(seeds({1})) == "1");
        assert(s.call(seeds({2})) == "0");
        assert(s.m.inserts == 4 && s.m.replaced == 3);
    }
    {   // N = 2, three keys: at least two share a slot
        Scenario s("n2", 2, 320, 64, 0);
        s.call(seeds({1, 2, 3}));
        s.call(seeds({1, 2, 3}));
        s.call(seeds({3, 2, 1}));
        s.call(seeds({3, 2, 1}));
        assert(s.m.table.size() <= 2);
    }
    {   // in-call duplicates: all miss, one entry
        Scenario s("dups", 64, 75, 64, 0);
        assert(s.call(seeds({7, 7, 7, 8})) == "0000");
        assert(s.m.inserts == 2);
        assert(s.call(seeds({7, 8, 7})) == "111");
    }
    {   // two rows of one call racing for one slot: the lowest row wins
        Scenario s("race", 1, 75, 64, 0);
        assert(s.call(seeds({1, 2})) == "00");
        assert(s.m.inserts == 1);
        assert(s.call(seeds({2})) == "0");
        assert(s.call(seeds({2, 1})) == "10");
        assert(s.call(seeds({1})) == "1");
    }
    {   // tag bits 0, N = 1: every probe passes the filter, the compare alone separates the keys
        Scenario s("bits0", 1, 75, 0, 0);
        const Row seq[] = {{9, 0, 'n'}, {9, 0, 'f'}, {9, 0, 'n'}, {9, 74, 'f'}, {9, 0, 'n'}, {9, 37, 'f'}, {9, 0, 'c'}, {9, 0, 'z'}};
        for (const Row& r : seq) assert(s.call({r}) == "0");
        assert(s.call({Row{9, 0, 'z'}}) == "1");
    }
    {   // chunks of 2 over 5 rows: chunk k hits what chunk k - 1 inserted
        Scenario s("chunk2", 65536, 75, 64, 2);
        assert(s.call(seeds({1, 2, 1, 2, 1})) == "00111");
        assert(s.call(seeds({3, 3, 3, 4, 4})) == "00101");
    }
    {   // a flush between calls
        Scenario s("flush", 64, 320, 64, 0);
        assert(s.call(seeds({1, 2, 3})) == "000");
        s.flush();
        assert(s.call(seeds({1, 2, 3})) == "000");
        assert(s.call(seeds({1, 2, 3})) == "111");
        assert(s.m.replaced == 0 && s.m.flushes == 1);
    }
}

int main() {
    check_hashes();
    check_model();
    printf("eval cache host check passed\n");
    return 0;
}
