// Index arithmetic of the streaming backward's LDS ring (rollout_bwd_cp_kernel.h, MODE = kCpStream) in one host-compilable place:
// plain constexpr functions, no HIP types.  The kernel uses them, and so does tools/stream_ring_model.cpp, which walks every
// interleaving of the workgroup's waves over the ring's counters.
//
// Steps are numbered by ORDINAL in the order the computing wave takes them (ordinal 0 = the last time step).  The fetching waves (two or three)
// write them in batches of `batch` consecutive ordinals, taking turns batch by batch; the ring has `slots` places, slots % batch == 0.
// Counters: `published` = ordinals [0, published) are in the ring, advanced in order; `answered` = the computing wave is done with
// ordinals [0, answered) -- it has read them and, in the hand-off form, written each one's answer (its two cell-gradient products)
// back into the slot it read the step from.
#pragma once

namespace mf {
namespace stream_ring {

// the ring slot ordinal o is written to and read from
constexpr int slot_of(int o, int slots) { return o % slots; }

// the fetching wave (0 / 1) that writes ordinal o: batches alternate, the trailing partial batch included
constexpr int owner_of(int o, int batch) { return (o / batch) & 1; }

// ... with `fetchers` fetching waves: wave k takes the batches k, k + fetchers, ...  (Three -- the twelve-slot hand-off kernels launched with
// 256 threads -- are modelled and were built, tools/experiments/stream_three_fetchers.patch; measured slower)
constexpr int owner_of(int o, int batch, int fetchers) { return (o / batch) % fetchers; }

// the number of fetching waves of a workgroup of `threads` threads: every wave but the computing one
constexpr int fetchers_of(int threads) { return threads / 64 - 1; }

// whole batches wave k of `fetchers` writes out of n_full, and the wave that writes the trailing partial batch
constexpr int batches_of(int n_full, int k, int fetchers) { return (n_full - k + fetchers - 1) / fetchers; }
constexpr int tail_owner(int n_full, int fetchers) { return n_full % fetchers; }

// true when a slot never changes hands: then the wave that writes ordinal o also wrote the ordinal it overwrites (the hand-off does NOT need it:
// the wave about to overwrite a slot reads the answer in it, behind has_room -- whichever wave wrote the step)
constexpr bool fixed_ownership(int slots, int batch) { return (slots / batch) % 2 == 0; }

// the room condition: ordinal o may be written once the ordinal it overwrites, o - slots, has been answered
constexpr bool has_room(int o, int answered, int slots) { return o + 1 - answered <= slots; }

// the ordinal whose answer a slot holds when ordinal o is about to be written into it (negative: none, the slot's initial contents)
constexpr int answer_in_slot(int o, int slots) { return o - slots; }

// the first ordinal nothing is ever written over: the answers of [first_undrained, n_steps) are collected after the last write
constexpr int first_undrained(int n_steps, int slots) { return n_steps > slots ? n_steps - slots : 0; }

// ---- the answer ring ----
// A variant of the hand-off that no kernel is built with at present: it was measured slower (the kernel change is
// kept as tools/experiments/stream_answer_ring.patch, the protocol stays modelled in tools/stream_ring_model.cpp).
// The answers do not travel through the coefficient slots there but through a ring of their own with `entries` places: the computing
// wave stores the answer of ordinal o into entry entry_of(o), and the fetching wave that writes ordinal o reads the entry it is about to
// reuse -- the answer of ordinal o - entries, its own step when fixed_ownership(entries, batch) -- in put(o), and what nothing was
// written over (first_undrained(n_steps, entries) onwards) after its last step.  A coefficient slot is then free as soon as it has
// been READ: the counter is "steps read" again (has_room with read in place of answered).
constexpr int entry_of(int o, int entries) { return o % entries; }

// the ordinal whose answer entry_of(o) holds when ordinal o is about to be written (negative: none, the entry's initial contents)
constexpr int answer_in_entry(int o, int entries) { return o - entries; }

// The computing wave counts `read = c` only after the chains of all ordinals <= c - kReadLead have stored their answers (a trip grabs
// its two steps, counts them, and only then runs the second chain; the step grabbed last has not begun).
constexpr int kReadLead = 3;

// the last ordinal whose answer is certainly stored once room for ordinal o has been granted: the grant means read >= o + 1 - slots
constexpr int last_answer_visible(int o, int slots) { return o + 1 - slots - kReadLead; }

// true when the answer a fetching wave reads in put(o) is there by construction, so that the wave never waits for it: LDS runs one
// wave's operations in order, and the computing wave's counter store follows its answer stores
constexpr bool answer_visible_at_put(int entries, int slots) { return answer_in_entry(0, entries) <= last_answer_visible(0, slots); }

}  // namespace stream_ring
}  // namespace mf
