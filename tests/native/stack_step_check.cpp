// The pooled traversal step's stack bookkeeping (csrc/dev_traversal.h), restated on the host in its two forms and held against each
// other exhaustively for the node step: the branchy transition (push_far_lds / pop_lds / SPC_TRAV_POP_ / SPC_STACK_DECODE, the step of the plain
// instantiation with its HBM part left out) and the straight-line one of the LDS-only instantiation (TravStack::top_lds / next_flat,
// SPC_STACK_DECODE_SEL).  tests/test_stack_step_host.py builds this with -fsanitize=address,undefined and runs it on the CPU.
//
// A lane's column is a heap block of exactly STACK_LDS = 16 words, so an access outside it is AddressSanitizer's to report; every
// index is checked against 0 .. 15 as well, and the straight-line form is only ever entered with sp + 3 <= 16, the guarantee of
// trace_pool's vote.  Compared after every transition: sp, node, leaf_count, `finished` and the words below sp.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

static constexpr int STACK_LDS = 16;
static constexpr int kTravDone = 0x7fffffff;
static constexpr uint32_t MISS = 0xffffffffu;

static long g_accesses = 0;
struct Column {
    uint32_t* e;
    Column() : e((uint32_t*)malloc(STACK_LDS * sizeof(uint32_t))) {}
    ~Column() { free(e); }
    Column(const Column&) = delete;
    uint32_t& at(int i) {
        if (i < 0 || i >= STACK_LDS) { printf("index %d outside the column\n", i); exit(2); }
        g_accesses++;
        return e[i];
    }
};
struct State {
    int sp, node, leaf_count;
    bool finished;
};

// ---- the branchy form -------------------------------------------------------------------------------------------------------
static void decode(uint32_t w, int& node, int& leaf) {
    if (w & 0x80000000u) { node = ~(int)((w & 0x7fffffffu) >> 3); leaf = (int)(w & 7u); }
    else node = (int)w;
}
static void push_far_lds(Column& c, int& sp, uint32_t r1, bool c1, uint32_t r2, bool c2, uint32_t r3, bool c3) {
    if (c3) c.at(sp) = r3;
    const int p2 = sp + (c3 ? 1 : 0);
    if (c2) c.at(p2) = r2;
    const int p1 = p2 + (c2 ? 1 : 0);
    if (c1) c.at(p1) = r1;
    sp = p1 + (c1 ? 1 : 0);
}
static void trav_pop(Column& c, State& s) {
    if (s.sp == 0) s.node = kTravDone;
    else { s.sp--; const uint32_t w = c.at(s.sp); decode(w, s.node, s.leaf_count); }
}
static void node_step_branchy(Column& c, State& s, const uint32_t k[4], const uint32_t r[4]) {
    if (k[0] == MISS) trav_pop(c, s);
    else {
        push_far_lds(c, s.sp, r[1], k[1] != MISS, r[2], k[2] != MISS, r[3], k[3] != MISS);
        decode(r[0], s.node, s.leaf_count);
    }
    s.finished = s.node == kTravDone;
}

// ---- the straight-line form ---------------------------------------------------------------------------------------------------
static void decode_sel(uint32_t w, int& node, int& leaf) {
    const bool lf = (w & 0x80000000u) != 0u;
    node = lf ? ~(int)((w & 0x7fffffffu) >> 3) : (int)w;
    leaf = lf ? (int)(w & 7u) : leaf;
}
static uint32_t top_lds(Column& c, int sp) { return c.at(sp > 0 ? sp - 1 : 0); }
static uint32_t next_flat(Column& c, int& sp, uint32_t top, bool miss, uint32_t r0, uint32_t r1, bool c1, uint32_t r2, bool c2, uint32_t r3, bool c3) {
    c.at(sp) = r3;
    const int p2 = sp + (c3 ? 1 : 0);
    c.at(p2) = r2;
    const int p1 = p2 + (c2 ? 1 : 0);
    c.at(p1) = r1;
    const uint32_t popped = sp == 0 ? (uint32_t)kTravDone : top;
    sp = miss ? (sp > 0 ? sp - 1 : 0) : p1 + (c1 ? 1 : 0);
    return miss ? popped : r0;
}
static void node_step_flat(Column& c, State& s, const uint32_t k[4], const uint32_t r[4]) {
    const uint32_t top = top_lds(c, s.sp);
    const uint32_t w = next_flat(c, s.sp, top, k[0] == MISS, r[0], r[1], k[1] != MISS, r[2], k[2] != MISS, r[3], k[3] != MISS);
    decode_sel(w, s.node, s.leaf_count);
    s.finished = s.node == kTravDone;
}
// ---- the cases ------------------------------------------------------------------------------------------------------------------
static uint32_t word(int kind, int salt) {   // 0 inner, 1 leaf of 1 .. 4 triangles, 2 empty leaf
    if (kind == 0) return (uint32_t)(1 + salt);
    return 0x80000000u | ((uint32_t)(100 + 4 * salt) << 3) | (kind == 1 ? (uint32_t)(1 + salt % 4) : 0u);
}
static void fill(Column& c, int sp, int top_kind) {
    for (int i = 0; i < STACK_LDS; i++) c.e[i] = 0xdead0000u + (uint32_t)i;   // above sp: never a word the traversal may follow
    for (int i = 0; i < sp; i++) c.e[i] = word((top_kind + (sp - 1 - i)) % 3, 7 + i);
}
static long g_cases = 0;
static void same(const char* what, const Column& a, const State& x, const Column& b, const State& y, int sp0) {
    g_cases++;
    bool ok = x.sp == y.sp && x.node == y.node && x.leaf_count == y.leaf_count && x.finished == y.finished;
    ok = ok && x.sp >= 0 && x.sp <= STACK_LDS && x.sp <= sp0 + 3;
    for (int i = 0; ok && i < x.sp; i++) ok = a.e[i] == b.e[i];
    if (!ok) {
        printf("%s differs: sp %d/%d node %d/%d leaf %d/%d finished %d/%d (start sp %d)\n", what, x.sp, y.sp, x.node, y.node,
               x.leaf_count, y.leaf_count, (int)x.finished, (int)y.finished, sp0);
        exit(1);
    }
}

int main() {
    Column a, b;
    // node step: all 16 hit patterns x three orders of the hits' distances x the kind of each child word x sp 0 .. 13 x the kind of the top
    static const int order[3][4] = {{0, 1, 2, 3}, {3, 2, 1, 0}, {2, 0, 3, 1}};
    for (int pat = 0; pat < 16; pat++)
        for (int od = 0; od < 3; od++)
            for (int kinds = 0; kinds < 81; kinds++)
                for (int sp = 0; sp + 3 <= STACK_LDS; sp++)
                    for (int tk = 0; tk < 3; tk++)
                        for (int lc0 = 0; lc0 <= 4; lc0 += 4) {
                            uint32_t key[4], ref[4], k[4], r[4];
                            for (int i = 0, q = kinds; i < 4; i++, q /= 3) {
                                ref[i] = word(q % 3, 20 + i);
                                float t = 1.0f + (float)order[od][i];
                                uint32_t tb;
                                memcpy(&tb, &t, 4);
                                key[i] = ((pat >> i) & 1) ? ((tb & ~3u) | (uint32_t)i) : MISS;
                            }
                            // the sort of SPC_NODE_STEP_Q: five compare-exchanges, misses last; then the refs by the keys' slot bits
                            memcpy(k, key, sizeof k);
                            auto cswap = [&](int i, int j) { const uint32_t lo = k[i] < k[j] ? k[i] : k[j], hi = k[i] < k[j] ? k[j] : k[i]; k[i] = lo; k[j] = hi; };
                            cswap(0, 1); cswap(2, 3); cswap(0, 2); cswap(1, 3); cswap(1, 2);
                            for (int i = 0; i < 4; i++) r[i] = ref[k[i] & 3u];
                            fill(a, sp, tk); fill(b, sp, tk);
                            State x = {sp, 3, lc0, false}, y = x;
                            node_step_branchy(a, x, k, r);
                            node_step_flat(b, y, k, r);
                            same("node step", a, x, b, y, sp);
                        }
    printf("ok %ld transitions, %ld column accesses\n", g_cases, g_accesses);
    return 0;
}
