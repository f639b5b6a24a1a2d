// The connect phase's job list (csrc/job_order.h), instantiated on the host: job_list_by_kind is the function the eye kernel calls,
// here with a wave that is replayed lane by lane.  tests/test_job_order_host.py builds this with -fsanitize=address,undefined and
// runs it on the CPU.
//
// A wave is 64 lanes that call the function in lock step; its only collective is the ballot.  The host runs the function once per
// lane with a wave that RECORDS each lane's vote (the vote of a step depends on the lane's own two words alone), then once more
// per lane with a wave that REPLAYS the collected masks.  The list is a heap block of exactly 3 x 64 bytes, so a write outside it
// is AddressSanitizer's to report; the recording pass writes into a block of its own.
// Checked for every case: the list is a permutation of exactly the live slots, general jobs stand before emitter jobs, each group
// is in (connection, lane) order, every lane returns the same count, and nothing behind the count is written.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "../../spcbpt-optix7_amd/csrc/job_order.h"

static constexpr int N = 3, SLOTS = N * 64;
static constexpr int STEPS = 2 * N;   // ballots per call: two sweeps over the connections

struct HostWave {
    unsigned long long* masks;
    uint32_t lane;
    bool replay;
    int step = 0;
    unsigned long long ballot(bool b) {
        if (step >= STEPS) { printf("more than %d ballots\n", STEPS); exit(2); }
        if (replay) return masks[step++];
        if (b) masks[step] |= 1ull << lane;
        step++;
        return 0ull;
    }
};

static long g_cases = 0;

static void check(const bool live[SLOTS], const bool emitter[SLOTS], const char* what) {
    uint32_t my_live[64], my_emitter[64];
    for (uint32_t lane = 0; lane < 64; lane++) {
        my_live[lane] = my_emitter[lane] = 0u;
        for (int it = 0; it < N; it++) {
            if (live[it * 64 + lane]) my_live[lane] |= 1u << it;
            if (emitter[it * 64 + lane]) my_emitter[lane] |= 1u << it;   // (also set on dead slots: the builder must not look at them)
        }
    }
    unsigned long long masks[STEPS] = {};
    uint8_t* scratch = (uint8_t*)malloc(SLOTS);
    for (uint32_t lane = 0; lane < 64; lane++) {
        HostWave wv{masks, lane, false};
        spc::job_list_by_kind<N>(wv, lane, my_live[lane], my_emitter[lane], scratch);
    }
    free(scratch);
    uint8_t* job = (uint8_t*)malloc(SLOTS);
    int16_t written[SLOTS];
    memset(job, 0xee, SLOTS);
    uint32_t n_jobs = 0;
    for (uint32_t lane = 0; lane < 64; lane++) {
        HostWave wv{masks, lane, true};
        const uint32_t n = spc::job_list_by_kind<N>(wv, lane, my_live[lane], my_emitter[lane], job);
        if (lane != 0 && n != n_jobs) { printf("%s: lane %u returns %u jobs, lane 0 %u\n", what, lane, n, n_jobs); exit(1); }
        n_jobs = n;
    }
    // the expected list, from the definition
    int want[SLOTS], n_want = 0;
    for (int kind = 0; kind < 2; kind++)
        for (int s = 0; s < SLOTS; s++)
            if (live[s] && (int)emitter[s] == kind) want[n_want++] = s;
    if ((int)n_jobs != n_want) { printf("%s: %u jobs, want %d\n", what, n_jobs, n_want); exit(1); }
    for (int j = 0; j < n_want; j++)
        if (job[j] != want[j]) { printf("%s: job %d is slot %d, want %d\n", what, j, (int)job[j], want[j]); exit(1); }
    for (int j = n_want; j < SLOTS; j++)
        if (job[j] != 0xee) { printf("%s: entry %d behind the list was written\n", what, j); exit(1); }
    // ... and the properties themselves, independently of `want`: a permutation of the live slots, kinds grouped, groups ascending
    memset(written, 0, sizeof written);
    bool seen_emitter = false;
    int prev = -1;
    for (uint32_t j = 0; j < n_jobs; j++) {
        const int s = job[j];
        if (s >= SLOTS || !live[s] || written[s]) { printf("%s: job %u = slot %d is dead, repeated or out of range\n", what, j, s); exit(1); }
        written[s] = 1;
        if (emitter[s] && !seen_emitter) { seen_emitter = true; prev = -1; }
        if (!emitter[s] && seen_emitter) { printf("%s: a general job behind an emitter job\n", what); exit(1); }
        if (s <= prev) { printf("%s: group not in (connection, lane) order at job %u\n", what, j); exit(1); }
        prev = s;
    }
    for (int s = 0; s < SLOTS; s++)
        if (live[s] && !written[s]) { printf("%s: live slot %d is missing\n", what, s); exit(1); }
    free(job);
    g_cases++;
}

static uint32_t g_rng = 0x9e3779b9u;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5; return g_rng; }

// `count` live slots, the first ones in slot order or a seeded random choice; kinds: 0 all general, 1 all emitter, 2 alternating, 3 random
static void with_count(int count, bool scattered, int kinds) {
    bool live[SLOTS] = {}, emitter[SLOTS];
    if (!scattered) for (int s = 0; s < count; s++) live[s] = true;
    else for (int left = count; left > 0;) { const int s = (int)(rnd() % SLOTS); if (!live[s]) { live[s] = true; left--; } }
    for (int s = 0; s < SLOTS; s++) emitter[s] = kinds == 0 ? false : kinds == 1 ? true : kinds == 2 ? (s & 1) != 0 : (rnd() & 1u) != 0u;
    char what[96];
    snprintf(what, sizeof what, "%d jobs, %s, kinds %d", count, scattered ? "scattered" : "packed", kinds);
    check(live, emitter, what);
}

int main() {
    // no job, one, the round boundaries and the full pool
    for (int count : {0, 1, 63, 64, 65, 127, 128, 129, 191, 192})
        for (int scattered = 0; scattered < 2; scattered++)
            for (int kinds = 0; kinds < 4; kinds++) with_count(count, scattered != 0, kinds);
    // one lane only: each lane alone, with every combination of its three connections alive and of their kinds
    for (int lane = 0; lane < 64; lane++)
        for (int lv = 1; lv < 8; lv++)
            for (int em = 0; em < 8; em++) {
                bool live[SLOTS] = {}, emitter[SLOTS] = {};
                for (int it = 0; it < N; it++) { live[it * 64 + lane] = (lv >> it) & 1; emitter[it * 64 + lane] = (em >> it) & 1; }
                check(live, emitter, "one lane only");
            }
    // exactly 64 / 65 / 128 / 129 general jobs with emitter jobs behind them (the list's first emitter job on and next to a round boundary)
    for (int general : {64, 65, 128, 129})
        for (int emitters : {0, 1, 63}) {
            if (general + emitters > SLOTS) continue;
            bool live[SLOTS] = {}, emitter[SLOTS] = {};
            for (int left = general + emitters, k = 0; left > 0;) {
                const int s = (int)(rnd() % SLOTS);
                if (!live[s]) { live[s] = true; emitter[s] = k++ >= general; left--; }
            }
            check(live, emitter, "general jobs up to a round boundary");
        }
    // seeded random set: every density of live slots and of emitter kinds
    for (int k = 0; k < 4000; k++) {
        bool live[SLOTS], emitter[SLOTS];
        const uint32_t p_live = rnd() % 101, p_em = rnd() % 101;
        for (int s = 0; s < SLOTS; s++) { live[s] = rnd() % 100 < p_live; emitter[s] = rnd() % 100 < p_em; }
        check(live, emitter, "random");
    }
    printf("ok %ld lists\n", g_cases);
    return 0;
}
