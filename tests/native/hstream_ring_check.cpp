// The ring of a host-fed stream (spiht_amd/csrc/hstream_ring.h) against a model of its own, on the CPU: every order of
// input / submit / next that is legal -- and every call that is not, which must be refused and change nothing -- for depth 2,
// 3 and 4 over 50 steps.  The ring's state is a function of (steps issued, steps taken, a slot handed out), so every order
// is a path through those states: each state is visited once, from each every call is tried.  Then long random walks.
// A host program with its own main: tests/test_hoststream_cpu.py builds it with -fsanitize=address,undefined and runs it.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <deque>
#include <map>
#include <tuple>
#include <vector>

#include "../../spiht_amd/csrc/hstream_ring.h"

static int g_fail = 0;
#define EXPECT(cond, ...)                                  \
    do {                                                   \
        if (!(cond)) {                                     \
            if (g_fail < 20) {                             \
                fprintf(stderr, "%s:%d: ", __FILE__, __LINE__); \
                fprintf(stderr, __VA_ARGS__);              \
                fprintf(stderr, "\n");                     \
            }                                              \
            g_fail++;                                      \
        }                                                  \
    } while (0)

// What the ring must do, said without slots' states: a queue of submitted steps and who holds which slot.
struct Model {
    int depth;
    uint64_t issued = 0, taken = 0;
    bool handed = false;
    long holds[HsRing::MAX_DEPTH];       // the step whose data lies in the slot; -1: none yet
    bool result_live[HsRing::MAX_DEPTH];  // a result was taken from the slot and the slot not handed out since
    std::deque<int> queue;                // slots of the submitted steps, oldest first
    explicit Model(int d) : depth(d) {
        for (int i = 0; i < HsRing::MAX_DEPTH; i++) { holds[i] = -1; result_live[i] = false; }
    }
};

static bool same(const HsRing &a, const HsRing &b) {
    if (a.depth != b.depth || a.issued != b.issued || a.taken != b.taken || a.handed != b.handed) return false;
    for (int i = 0; i < HsRing::MAX_DEPTH; i++)
        if (a.st[i] != b.st[i] || a.step_of[i] != b.step_of[i]) return false;
    return true;
}

enum Op { OP_INPUT = 0, OP_SUBMIT = 1, OP_NEXT = 2, OP_PEEK = 3, OP_COUNT = 4 };  // PEEK: next's timeout path -- it looks, and leaves

// one call on ring and model; every expectation is checked
static void apply(HsRing &r, Model &m, int op) {
    const HsRing before = r;
    const int in_flight = (int)m.queue.size();
    EXPECT(r.in_flight() == in_flight, "in_flight %d, model %d", r.in_flight(), in_flight);
    EXPECT(r.full() == (in_flight == m.depth), "full() with %d of %d in flight", in_flight, m.depth);
    switch (op) {
    case OP_INPUT: {
        const int s = r.acquire();
        if (m.handed) {  // asked again: the same slot, nothing changes
            EXPECT(s == (int)(m.issued % (uint64_t)m.depth), "second input gave slot %d", s);
            EXPECT(same(before, r), "second input changed the ring");
        } else if (in_flight == m.depth) {  // busy
            EXPECT(s == -1, "input on a full ring gave slot %d", s);
            EXPECT(same(before, r), "refused input changed the ring");
        } else {
            EXPECT(s == (int)(m.issued % (uint64_t)m.depth), "input gave slot %d for step %llu", s, (unsigned long long)m.issued);
            if (s >= 0 && s < m.depth) {
                for (int q : m.queue) EXPECT(q != s, "slot %d handed out while its step is still submitted", s);
                EXPECT(before.st[s] == HsRing::FREE || before.st[s] == HsRing::TAKEN, "slot %d reused from state %d", s, (int)before.st[s]);
                EXPECT(m.holds[s] < 0 || (uint64_t)m.holds[s] < m.taken, "slot %d reused before step %ld was taken", s, m.holds[s]);
                m.result_live[s] = false;
                m.handed = true;
            }
        }
        EXPECT(r.handed_slot() == (m.handed ? (int)(m.issued % (uint64_t)m.depth) : -1), "handed_slot()");
        break;
    }
    case OP_SUBMIT: {
        const int s = r.submit();
        if (!m.handed) {
            EXPECT(s == -1, "submit without input gave slot %d", s);
            EXPECT(same(before, r), "refused submit changed the ring");
        } else {
            EXPECT(s == (int)(m.issued % (uint64_t)m.depth), "submit queued slot %d", s);
            if (s >= 0 && s < m.depth) {
                EXPECT(r.step_of[s] == m.issued, "slot %d holds step %llu, not %llu", s, (unsigned long long)r.step_of[s],
                       (unsigned long long)m.issued);
                m.holds[s] = (long)m.issued;
                m.queue.push_back(s);
            }
            m.issued++;
            m.handed = false;
        }
        break;
    }
    case OP_PEEK: {
        const int s = r.oldest();
        EXPECT(s == (m.queue.empty() ? -1 : m.queue.front()), "oldest() gave slot %d", s);
        EXPECT(same(before, r), "oldest() changed the ring");
        break;
    }
    default: {
        const int s = r.take();
        if (m.queue.empty()) {
            EXPECT(s == -1, "next with nothing submitted gave slot %d", s);
            EXPECT(same(before, r), "refused next changed the ring");
        } else {
            EXPECT(s == m.queue.front(), "next gave slot %d, the oldest step is on %d", s, m.queue.front());
            if (s >= 0 && s < m.depth) {
                EXPECT((uint64_t)m.holds[s] == m.taken, "results out of order: step %ld came out as number %llu", m.holds[s],
                       (unsigned long long)m.taken);
                EXPECT(r.st[s] == HsRing::TAKEN, "taken slot %d is in state %d", s, (int)r.st[s]);
                m.result_live[s] = true;
            }
            m.queue.pop_front();
            m.taken++;
        }
        break;
    }
    }
    // a result that was handed out stays: its slot is not submitted and not handed out until input gives it again
    for (int i = 0; i < m.depth; i++)
        if (m.result_live[i]) EXPECT(r.st[i] == HsRing::TAKEN, "slot %d lost its result (state %d)", i, (int)r.st[i]);
}

// every state (issued <= steps, in flight, handed) once; from each, every call
static long exhaustive(int depth, uint64_t steps) {
    typedef std::tuple<uint64_t, uint64_t, bool> Key;
    struct Node { HsRing r; Model m; };
    std::map<Key, bool> seen;
    std::vector<Node> todo;
    todo.push_back(Node{HsRing(depth), Model(depth)});
    seen[Key(0, 0, false)] = true;
    long edges = 0;
    while (!todo.empty()) {
        Node n = todo.back();
        todo.pop_back();
        for (int op = 0; op < OP_COUNT; op++) {
            Node k = n;
            apply(k.r, k.m, op);
            edges++;
            if (k.m.issued > steps) continue;
            const Key key(k.m.issued, k.m.taken, k.m.handed);
            if (!seen[key]) { seen[key] = true; todo.push_back(k); }
        }
    }
    // every state the rules allow was reached: in flight 0 .. depth, handed only while a slot is free
    long want = 0;
    for (uint64_t i = 0; i <= steps; i++)
        for (uint64_t t = (i > (uint64_t)depth ? i - (uint64_t)depth : 0); t <= i; t++) want += (i - t < (uint64_t)depth) ? 2 : 1;
    long got = 0;
    for (auto &kv : seen) got += kv.second ? 1 : 0;
    EXPECT(got == want, "depth %d: %ld states reached, %ld exist", depth, got, want);
    return edges;
}

static uint32_t lcg(uint32_t *s) { return *s = *s * 1664525u + 1013904223u; }

static void random_walk(int depth, uint32_t seed, int calls) {
    HsRing r(depth);
    Model m(depth);
    for (int i = 0; i < calls; i++) apply(r, m, (int)((lcg(&seed) >> 16) % OP_COUNT));
    // drain: what is submitted comes out, in order, and then nothing does
    while (!m.queue.empty()) apply(r, m, OP_NEXT);
    apply(r, m, OP_NEXT);
    EXPECT(r.oldest() == -1 && r.in_flight() == 0, "ring not empty after the drain");
}

int main() {
    EXPECT(!HsRing::depth_ok(1) && HsRing::depth_ok(2) && HsRing::depth_ok(4) && !HsRing::depth_ok(5), "depth_ok");
    long edges = 0;
    for (int depth = 2; depth <= 4; depth++) {
        edges += exhaustive(depth, 50);
        for (uint32_t seed = 1; seed <= 8; seed++) random_walk(depth, seed * 2654435761u + (uint32_t)depth, 4000);
        // the plain pipeline: fill, then one out one in for 50 steps -- busy exactly when `depth` are in flight
        HsRing r(depth);
        Model m(depth);
        for (int step = 0; step < 50; step++) {
            if ((int)m.queue.size() == depth) {
                apply(r, m, OP_INPUT);  // busy
                EXPECT(!m.handed, "input passed on a full ring");
                apply(r, m, OP_SUBMIT);  // refused
                apply(r, m, OP_PEEK);    // a timeout: looks and leaves
                apply(r, m, OP_NEXT);
            }
            apply(r, m, OP_INPUT);
            EXPECT(m.handed, "input refused with a free slot");
            apply(r, m, OP_SUBMIT);
        }
        EXPECT(m.issued == 50, "50 steps");
    }
    if (g_fail) {
        fprintf(stderr, "hstream_ring_check: %d failures\n", g_fail);
        return 1;
    }
    printf("hstream_ring_check ok: %ld transitions\n", edges);
    return 0;
}
