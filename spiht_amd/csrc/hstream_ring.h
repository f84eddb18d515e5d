// The bookkeeping of a host-fed stream's ring of slots (hoststream.cpp; include/spiht_hip.h: spiht_hstream_*).  Plain C++, no
// HIP: which slot is handed out, which are queued, which one comes out next and when a slot may be used again.
//
// A slot goes  free -> handed out (spiht_hstream_input) -> submitted (_submit) -> taken (_next) -> handed out again ...
// Slots are issued in ring order, step k on slot k % depth, and results leave in the order of submission, so the slot the
// next step needs is the one whose result has been waiting longest: the ring is full exactly when that slot is still
// submitted.  A taken slot is as good as a free one for _input; the difference is that what _next returned for it is valid
// until then.  One slot is handed out at a time.
#pragma once
#include <stdint.h>

struct HsRing {
    enum State : uint8_t { FREE = 0, HANDED = 1, SUBMITTED = 2, TAKEN = 3 };
    enum { MIN_DEPTH = 2, MAX_DEPTH = 4 };
    int depth = 0;
    State st[MAX_DEPTH] = {FREE, FREE, FREE, FREE};
    uint64_t step_of[MAX_DEPTH] = {0, 0, 0, 0};  // the step a submitted / taken slot holds
    uint64_t issued = 0;     // steps handed out and submitted so far: the next _input gives slot issued % depth
    uint64_t taken = 0;      // steps taken so far: the next _next takes step `taken`, on slot taken % depth
    bool handed = false;     // slot issued % depth is handed out and not submitted yet

    static bool depth_ok(int d) { return d >= MIN_DEPTH && d <= MAX_DEPTH; }
    explicit HsRing(int d = MIN_DEPTH) : depth(depth_ok(d) ? d : MIN_DEPTH) {}

    int in_flight() const { return (int)(issued - taken); }      // steps submitted and not taken
    bool full() const { return in_flight() == depth; }           // the slot the next step needs is still submitted
    int next_slot() const { return (int)(issued % (uint64_t)depth); }

    // _input: the slot for the next step, or -1 when the ring is full.  Asking again before the submit gives the same slot.
    int acquire() {
        const int s = next_slot();
        if (handed) return s;
        if (st[s] == SUBMITTED) return -1;
        st[s] = HANDED;
        handed = true;
        return s;
    }
    // the slot a _submit would queue, or -1: nothing is handed out
    int handed_slot() const { return handed ? next_slot() : -1; }
    // _submit: the handed-out slot becomes step `issued`; returns the slot, or -1 when nothing is handed out (no change)
    int submit() {
        if (!handed) return -1;
        const int s = next_slot();
        st[s] = SUBMITTED;
        step_of[s] = issued;
        handed = false;
        issued++;
        return s;
    }
    // the slot of the oldest submitted step, or -1 when nothing is submitted
    int oldest() const { return in_flight() > 0 ? (int)(taken % (uint64_t)depth) : -1; }
    // _next, once the oldest step is complete: its slot becomes taken; returns the slot, or -1 (no change)
    int take() {
        const int s = oldest();
        if (s < 0) return -1;
        st[s] = TAKEN;
        taken++;
        return s;
    }
};
