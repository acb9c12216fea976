// Model of the streaming backward's ring protocol (monoforce_amd/csrc/rollout_bwd_cp_kernel.h, MODE = kCpStream): the computing wave and
// the two (or three) fetching waves as state machines over the LDS counters -- published, answered, the snap flag -- and each wave's program
// position, with the index arithmetic of csrc/stream_ring.h (the header the kernel uses).  Every interleaving of the programs is
// explored (breadth first over the reachable states) for n_steps = 1 .. 30 (the answer ring: 1 .. 60, beyond two answer rings) and
// every ring the kernels are built with:
//   twelve slots, batches of three, hand-off   (the float32 default-integrator kernels: answers go back through the slots)
//   ... the same with THREE fetching waves     (not built: measured slower, DESIGN.md section 8, tools/experiments/stream_three_fetchers.patch --
//                                               those kernels launched with 256 threads: a slot changes hands -- ordinal o - 12 was written
//                                               by wave (owner(o) + 2) mod 3 -- and the answer in it is read by whoever writes ordinal o)
//   twelve slots, batches of three, answer ring (not built: measured slower, DESIGN.md section 8 -- "answered" is "read" again, the
//                                               answers go back through a ring of 24 entries of their own, written by the computing wave,
//                                               consumed by the step's owner in put(o + 24) and in the final drain; the kernel side is
//                                               tools/experiments/stream_answer_ring.patch)
//   six slots, batches of three / of two       (the other streaming kernels: "answered" is "read", nothing goes back)
//   six slots, batches of three, hand-off      (not built; ownership is fixed there too, so the protocol must hold)
// It fails (exit status 1, one line per finding) on
//   - a reachable state in which no wave can move before all are done,
//   - a slot overwritten before its answer was consumed, or answered after it was overwritten,
//   - an answer consumed twice, or never,
//   - out-of-order publication (a counter that moves past a step not yet written, or backwards),
//   - a blocked computing wave that has answered fewer than p - 2 steps (the invariant that rules out deadlock),
//   - answer ring: an entry read before its answer was written -- in put() that is a fetching wave that would have had to wait for an
//     answer in steady state, which the kernel does not do --, an entry handed to a new step before its answer was consumed, an answer
//     consumed twice, or never.
// With an argument the protocol is MUTATED, to show that the model sees a broken one (tests/test_stream_three_fetchers_cpu.py):
//   early-room   a fetching wave is granted room one slot early (has_room as if the ring had one slot more)
// Exit status 0, "explored <N> states" (the total) and one "...: explored <n> states" line per configuration otherwise.  Host only:  c++ -std=c++17 -O2 -I monoforce_amd/csrc tools/stream_ring_model.cpp
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <deque>
#include <string>
#include <unordered_set>
#include <vector>
#include "stream_ring.h"

namespace sr = mf::stream_ring;

enum OpKind : int {
  F_BATCH,      // a batch (or a trailing single step) begins: pub = arg
  F_ROOM,       // blocks until ordinal arg may be written
  F_TAKE,       // hand-off: read the old answer of the slot ordinal arg goes to (ordinal arg - slots)
  F_WRITE,      // write ordinal arg into its slot
  F_PUBTRY,     // publish [pub, arg) if it is this wave's turn
  F_PUBWAIT,    // publish [pub, arg): blocks until it is this wave's turn
  F_SNAP,       // fetching wave 1: the snap's cell is ready
  F_ALLDONE,    // hand-off: blocks until answered == n_steps
  F_DRAIN,      // hand-off: read the answer of ordinal arg, still in its slot
  C_ENSURE,     // blocks until arg more steps are published
  C_GRAB,       // read the next step out of its slot
  C_ANSWER,     // hand-off: write the answer of ordinal arg into its slot
  C_COUNT,      // answered = arg
  C_SNAPWAIT,   // blocks until the snap's cell is ready
  F_ATAKE,      // answer ring: read the entry ordinal arg will use (the answer of ordinal arg - entries), then leave arg's cell index there
  F_ALLANS,     // answer ring: blocks until the computing wave has stored its last answer
  F_ADRAIN,     // answer ring: read the answer of ordinal arg, still in its entry
  C_AANSWER,    // answer ring: write the answer of ordinal arg into its entry
  C_ALLANS,     // answer ring: all answers are stored
};
struct Op { int kind, arg; };

struct Config { int n_steps, slots, batch; bool handoff; int entries; int fetchers = 2; bool early_room = false; };      // entries > 0: the answer ring (then not `handoff`)

// The programs, in the kernel's own order of operations.
static std::vector<Op> fetcher_program(const Config& c, int fk) {
  std::vector<Op> p;
  auto put = [&](int o) {
    p.push_back({F_ROOM, o});
    if (c.handoff) p.push_back({F_TAKE, o});
    if (c.entries) p.push_back({F_ATAKE, o});
    p.push_back({F_WRITE, o});
    p.push_back({F_PUBTRY, o + 1});
  };
  const int n_full = c.n_steps / c.batch;
  if (sr::batches_of(n_full, fk, c.fetchers) != (n_full > fk ? (n_full - fk + c.fetchers - 1) / c.fetchers : 0)) std::printf("FINDING batches_of(%d, %d, %d)\n", n_full, fk, c.fetchers);
  for (int j = fk; j < n_full; j += c.fetchers) {
    p.push_back({F_BATCH, j * c.batch});
    for (int i = 0; i < c.batch; ++i) put(j * c.batch + i);
    p.push_back({F_PUBWAIT, (j + 1) * c.batch});
  }
  if (fk == sr::tail_owner(n_full, c.fetchers))
    for (int o = n_full * c.batch; o < c.n_steps; ++o) { p.push_back({F_BATCH, o}); put(o); p.push_back({F_PUBWAIT, o + 1}); }
  if (fk == 1) p.push_back({F_SNAP, 0});
  if (c.handoff) {
    p.push_back({F_ALLDONE, 0});
    for (int o = sr::first_undrained(c.n_steps, c.slots); o < c.n_steps; ++o)
      if (sr::owner_of(o, c.batch, c.fetchers) == fk) p.push_back({F_DRAIN, o});
  }
  if (c.entries) {
    p.push_back({F_ALLANS, 0});
    for (int o = sr::first_undrained(c.n_steps, c.entries); o < c.n_steps; ++o)
      if (sr::owner_of(o, c.batch, c.fetchers) == fk) p.push_back({F_ADRAIN, o});
  }
  return p;
}
static std::vector<Op> computer_program(const Config& c) {
  std::vector<Op> p;
  int consumed = 0;
  auto grab = [&]() { p.push_back({C_GRAB, consumed}); ++consumed; };
  auto finish = [&](int n) {      // the chain of step n is done (ordinal n_steps - 1 - n)
    if (c.handoff) p.push_back({C_ANSWER, c.n_steps - 1 - n});
    if (c.entries) p.push_back({C_AANSWER, c.n_steps - 1 - n});
  };
  auto release = [&]() { if (!c.handoff) p.push_back({C_COUNT, consumed}); };      // the old form: counted when read
  int n = c.n_steps - 1;
  p.push_back({C_ENSURE, 1}); grab(); release();
  for (; n >= 2; n -= 2) {
    p.push_back({C_ENSURE, 2});
    grab(); finish(n);
    grab(); release(); finish(n - 1);
    if (c.handoff) p.push_back({C_COUNT, c.n_steps - (n - 1)});
  }
  if (n == 1) {
    p.push_back({C_ENSURE, 1}); grab(); release(); finish(1);
    if (c.handoff) p.push_back({C_COUNT, c.n_steps - 1});
    n = 0;
  }
  finish(0);
  if (c.handoff) p.push_back({C_COUNT, c.n_steps});
  if (c.entries) p.push_back({C_ALLANS, 0});
  p.push_back({C_SNAPWAIT, 0});
  return p;
}

constexpr int kMaxSlots = 12, kMaxEntries = 24;
struct State {
  uint16_t pc[4];                 // fetching waves 0 .. fetchers - 1, then the computing wave
  int8_t published, answered, snap, consumed;
  int8_t pub[3];                  // a fetching wave's first written-but-unpublished ordinal
  int8_t ord[kMaxSlots];          // the ordinal a slot holds (-1: its initial contents)
  int8_t st[kMaxSlots];           // 0 written, 1 read by the computing wave, 2 answered, 3 answer consumed
  int8_t allans;                  // answer ring: the computing wave's "all answered" flag
  int8_t aord[kMaxEntries];       // answer ring: the ordinal an entry belongs to (-1: its initial contents)
  int8_t ast[kMaxEntries];        // 0 handed to its step (cell index there), 2 answered, 3 answer consumed
};
static std::string key(const State& s) { return std::string(reinterpret_cast<const char*>(&s), sizeof(State)); }

struct Result { long states = 0; int findings = 0; };

static void finding(Result& r, const Config& c, const char* what, int o) {
  if (r.findings < 20)
    std::printf("FINDING n_steps %d slots %d batch %d fetchers %d %s: %s (ordinal %d)\n", c.n_steps, c.slots, c.batch, c.fetchers,
                c.entries ? "answer ring" : (c.handoff ? "hand-off" : "read-counted"), what, o);
  ++r.findings;
}

static Result explore(const Config& c) {
  Result res;
  const int nw = c.fetchers + 1;
  std::vector<Op> prog[4];
  for (int k = 0; k < c.fetchers; ++k) prog[k] = fetcher_program(c, k);
  prog[c.fetchers] = computer_program(c);
  State s0;
  std::memset(&s0, 0, sizeof(s0));
  for (int i = 0; i < kMaxSlots; ++i) { s0.ord[i] = -1; s0.st[i] = 3; }
  for (int i = 0; i < kMaxEntries; ++i) { s0.aord[i] = -1; s0.ast[i] = 3; }
  std::unordered_set<std::string> seen;
  std::deque<State> todo;
  seen.insert(key(s0)); todo.push_back(s0);
  while (!todo.empty()) {
    const State s = todo.front(); todo.pop_front();
    ++res.states;
    bool all_done = true, moved = false;
    for (int w = 0; w < nw; ++w) {
      if (s.pc[w] >= prog[w].size()) continue;
      all_done = false;
      const Op op = prog[w][s.pc[w]];
      State t = s;
      bool blocked = false;
      const int sl = op.arg >= 0 ? sr::slot_of(op.arg, c.slots) : 0;
      switch (op.kind) {
        case F_BATCH: t.pub[w] = (int8_t)op.arg; break;
        case F_ROOM: blocked = !sr::has_room(op.arg, s.answered, c.slots + (c.early_room ? 1 : 0)); break;
        case F_TAKE: {
          const int old = sr::answer_in_slot(op.arg, c.slots);
          if (old >= 0) {
            // (two fetching waves on these rings: a slot stays with one wave; three: it does not, and need not -- stream_ring.h)
            if (c.fetchers == 2 && sr::owner_of(old, c.batch) != w) finding(res, c, "an answer read by the wave that did not write the step", old);
            if (c.fetchers == 3 && sr::owner_of(old, c.batch, 3) != (w + 2) % 3 && c.slots == 12 && c.batch == 3) finding(res, c, "an answer read by an unexpected wave", old);
            if (s.ord[sl] != old || s.st[sl] < 2) finding(res, c, "an answer read before it was written", old);
            else if (s.st[sl] == 3) finding(res, c, "an answer consumed twice", old);
            t.st[sl] = 3;
          } else if (s.ord[sl] != -1) finding(res, c, "initial contents expected", op.arg);
          break;
        }
        case F_WRITE: {
          const int old = s.ord[sl];
          if (old >= 0 && old != sr::answer_in_slot(op.arg, c.slots)) finding(res, c, "a slot holds an unexpected step", old);
          if (old >= 0 && s.st[sl] < (c.handoff ? 3 : 1)) finding(res, c, c.handoff ? "a slot overwritten before its answer was consumed" : "a slot overwritten before it was read", old);
          t.ord[sl] = (int8_t)op.arg; t.st[sl] = 0;
          break;
        }
        case F_PUBTRY:
        case F_PUBWAIT: {
          const bool turn = s.published == s.pub[w];
          if (!turn && op.kind == F_PUBWAIT && s.pub[w] != op.arg) { blocked = true; break; }
          if (turn && s.pub[w] != op.arg) {
            if (op.arg <= s.published) finding(res, c, "publication moves backwards", op.arg);
            for (int o = s.published; o < op.arg; ++o)
              if (s.ord[sr::slot_of(o, c.slots)] != o) finding(res, c, "published before written", o);
            t.published = (int8_t)op.arg; t.pub[w] = (int8_t)op.arg;
          }
          break;
        }
        case F_SNAP: t.snap = 1; break;
        case F_ALLDONE: blocked = s.answered != c.n_steps; break;
        case F_DRAIN:
          if (s.ord[sl] != op.arg || s.st[sl] < 2) finding(res, c, "a drained answer is not there", op.arg);
          else if (s.st[sl] == 3) finding(res, c, "an answer consumed twice", op.arg);
          t.st[sl] = 3;
          break;
        case C_ENSURE:
          blocked = s.published < s.consumed + op.arg;
          if (blocked && c.handoff) {      // blocked on ordinals up to p = consumed + arg - 1: the invariant beside room()
            const int p = s.consumed + op.arg - 1;
            if (s.answered < p - 2) finding(res, c, "a blocked computing wave has answered fewer than p - 2 steps", p);
          }
          break;
        case C_GRAB:
          if (op.arg >= s.published) finding(res, c, "a step read before it was published", op.arg);
          if (s.ord[sl] != op.arg || s.st[sl] != 0) finding(res, c, "a step read that is not in its slot", op.arg);
          t.st[sl] = 1; t.consumed = (int8_t)(op.arg + 1);
          break;
        case C_ANSWER:
          if (s.ord[sl] != op.arg) finding(res, c, "an answer written into a slot that was overwritten", op.arg);
          else if (s.st[sl] != 1) finding(res, c, "an answer written twice or before the step was read", op.arg);
          t.st[sl] = 2;
          break;
        case C_COUNT:
          if (op.arg < s.answered) finding(res, c, "the answered counter moves backwards", op.arg);
          t.answered = (int8_t)op.arg;
          break;
        case C_SNAPWAIT: blocked = !s.snap; break;
        case F_ATAKE: {
          const int e = sr::entry_of(op.arg, c.entries), old = sr::answer_in_entry(op.arg, c.entries);
          if (old >= 0) {
            if (sr::owner_of(old, c.batch) != w) finding(res, c, "an answer read by the wave that did not write the step", old);
            if (s.aord[e] != old) finding(res, c, "an answer entry holds an unexpected step", old);
            else if (s.ast[e] < 2) finding(res, c, "a fetching wave would have had to wait for an answer: its entry read in put() before it was written", old);
            else if (s.ast[e] == 3) finding(res, c, "an answer consumed twice", old);
            if (old > sr::last_answer_visible(op.arg, c.slots)) finding(res, c, "an answer read in put() beyond stream_ring's visibility bound", old);
          } else if (s.aord[e] != -1) finding(res, c, "initial contents expected in an answer entry", op.arg);
          if (s.ast[e] < 3 && s.aord[e] >= 0 && s.aord[e] != old) finding(res, c, "an answer entry handed on before its answer was consumed", s.aord[e]);
          t.aord[e] = (int8_t)op.arg; t.ast[e] = 0;
          break;
        }
        case F_ALLANS: blocked = !s.allans; break;
        case F_ADRAIN: {
          const int e = sr::entry_of(op.arg, c.entries);
          if (s.aord[e] != op.arg || s.ast[e] < 2) finding(res, c, "a drained answer entry read before it was written", op.arg);
          else if (s.ast[e] == 3) finding(res, c, "an answer consumed twice", op.arg);
          t.ast[e] = 3;
          break;
        }
        case C_AANSWER: {
          const int e = sr::entry_of(op.arg, c.entries);
          if (s.aord[e] != op.arg) finding(res, c, "an answer written into an entry that was handed on (or never handed to its step)", op.arg);
          else if (s.ast[e] != 0) finding(res, c, "an answer written twice", op.arg);
          if (op.arg >= s.consumed) finding(res, c, "an answer written before the step was read", op.arg);
          t.ast[e] = 2;
          break;
        }
        case C_ALLANS: t.allans = 1; break;
      }
      if (blocked) continue;
      moved = true;
      ++t.pc[w];
      if (seen.insert(key(t)).second) todo.push_back(t);
    }
    if (!all_done && !moved) finding(res, c, "no wave can move", s.published);
    if (all_done) {
      if (s.published != c.n_steps || s.answered != c.n_steps) finding(res, c, "the counters do not end at n_steps", s.published);
      if (c.handoff)
        for (int o = sr::first_undrained(c.n_steps, c.slots); o < c.n_steps; ++o)
          if (s.st[sr::slot_of(o, c.slots)] != 3) finding(res, c, "an answer never consumed", o);
      if (c.entries)      // (the ordinals before first_undrained were consumed in put(): an entry is handed on only behind that check)
        for (int o = sr::first_undrained(c.n_steps, c.entries); o < c.n_steps; ++o)
          if (s.aord[sr::entry_of(o, c.entries)] != o || s.ast[sr::entry_of(o, c.entries)] != 3) finding(res, c, "an answer never consumed", o);
    }
    if (res.findings > 100) break;
  }
  return res;
}

int main(int argc, char** argv) {
  const bool early_room = argc > 1 && std::strcmp(argv[1], "early-room") == 0;
  if (argc > 1 && !early_room) { std::printf("usage: %s [early-room]\n", argv[0]); return 2; }
  static_assert(sr::fixed_ownership(12, 3) && sr::fixed_ownership(6, 3) && !sr::fixed_ownership(6, 2), "ring ownership");
  static_assert(sr::owner_of(8, 3, 3) == 2 && sr::owner_of(9, 3, 3) == 0 && sr::owner_of(5, 3, 2) == sr::owner_of(5, 3) && sr::fetchers_of(256) == 3 && sr::fetchers_of(192) == 2 &&
                sr::batches_of(7, 1, 3) == 2 && sr::batches_of(7, 0, 2) == 4 && sr::tail_owner(7, 3) == 1, "three fetching waves");
  static_assert(sr::slot_of(13, 12) == 1 && sr::owner_of(5, 3) == 1 && sr::owner_of(6, 3) == 0 && sr::has_room(11, 0, 12) && !sr::has_room(12, 0, 12), "ring arithmetic");
  static_assert(sr::fixed_ownership(24, 3) && sr::entry_of(25, 24) == 1 && sr::answer_in_entry(30, 24) == 6 && sr::first_undrained(30, 24) == 6, "answer ring arithmetic");
  static_assert(sr::answer_visible_at_put(24, 12) && sr::answer_visible_at_put(18, 12) && !sr::answer_visible_at_put(12, 12), "answer ring: visibility bound");
  const struct { int slots, batch; bool handoff; int entries, horizons; const char* name; int fetchers; } rings[] = {
      {12, 3, true, 0, 30, "12 slots, batches of 3, hand-off", 2},      {6, 3, true, 0, 30, "6 slots, batches of 3, hand-off", 2},
      {12, 3, false, 0, 30, "12 slots, batches of 3, read-counted", 2}, {6, 3, false, 0, 30, "6 slots, batches of 3, read-counted", 2},
      {6, 2, false, 0, 30, "6 slots, batches of 2, read-counted", 2},   {12, 3, false, 24, 60, "12 slots, batches of 3, read-counted, answer ring of 24", 2},
      {12, 3, true, 0, 30, "12 slots, batches of 3, hand-off, three fetching waves", 3}};
  constexpr int kRings = (int)(sizeof(rings) / sizeof(rings[0]));
  long states = 0, per_ring[kRings] = {};
  int findings = 0;
  for (int k = 0; k < kRings; ++k)
    for (int n = 1; n <= rings[k].horizons; ++n) {
      if (early_room && !rings[k].handoff) continue;      // (the mutation is shown on the hand-off rings)
      const Result x = explore(Config{n, rings[k].slots, rings[k].batch, rings[k].handoff, rings[k].entries, rings[k].fetchers, early_room});
      states += x.states; per_ring[k] += x.states; findings += x.findings;
    }
  if (findings) { std::printf("%d findings\n", findings); return 1; }
  std::printf("explored %ld states\n", states);
  // (the three-fetcher ring's line ends differently: the lines of the rings the kernels are built with keep their count)
  for (int k = 0; k < kRings; ++k)
    std::printf(rings[k].fetchers == 2 ? "%s, n_steps 1 .. %d: explored %ld states\n" : "%s, n_steps 1 .. %d: explored %ld states (four programs)\n", rings[k].name, rings[k].horizons, per_ring[k]);
  return 0;
}
