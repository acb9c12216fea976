// Index arithmetic of the streaming backward's LDS ring (rollout_bwd_cp_kernel.h, MODE = kCpStream) in one host-compilable place:
// plain constexpr functions, no HIP types.  The kernel uses them, and so does tools/stream_ring_model.cpp, which walks every
// interleaving of the three waves over the ring's counters.
//
// Steps are numbered by ORDINAL in the order the computing wave takes them (ordinal 0 = the last time step).  The two fetching waves
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

// true when a slot never changes hands: then the wave that writes ordinal o also wrote the ordinal it overwrites (hand-off needs it)
constexpr bool fixed_ownership(int slots, int batch) { return (slots / batch) % 2 == 0; }

// the room condition: ordinal o may be written once the ordinal it overwrites, o - slots, has been answered
constexpr bool has_room(int o, int answered, int slots) { return o + 1 - answered <= slots; }

// the ordinal whose answer a slot holds when ordinal o is about to be written into it (negative: none, the slot's initial contents)
constexpr int answer_in_slot(int o, int slots) { return o - slots; }

// the first ordinal nothing is ever written over: the answers of [first_undrained, n_steps) are collected after the last write
constexpr int first_undrained(int n_steps, int slots) { return n_steps > slots ? n_steps - slots : 0; }

}  // namespace stream_ring
}  // namespace mf
