// Model of the streaming backward's ring protocol (monoforce_amd/csrc/rollout_bwd_cp_kernel.h, MODE = kCpStream): the computing wave and
// the two fetching waves as state machines over the LDS counters -- published, answered, the snap flag -- and each wave's program
// position, with the index arithmetic of csrc/stream_ring.h (the header the kernel uses).  Every interleaving of the three programs is
// explored (breadth first over the reachable states) for n_steps = 1 .. 30 and every ring the kernels are built with:
//   twelve slots, batches of three, hand-off   (the float32 default-integrator kernels: answers go back through the slots)
//   six slots, batches of three / of two       (the other streaming kernels: "answered" is "read", nothing goes back)
//   six slots, batches of three, hand-off      (not built; ownership is fixed there too, so the protocol must hold)
// It fails (exit status 1, one line per finding) on
//   - a reachable state in which no wave can move before all three are done,
//   - a slot overwritten before its answer was consumed, or answered after it was overwritten,
//   - an answer consumed twice, or never,
//   - out-of-order publication (a counter that moves past a step not yet written, or backwards),
//   - a blocked computing wave that has answered fewer than p - 2 steps (the invariant that rules out deadlock).
// Exit status 0 and "explored <N> states" otherwise.  Host only:  c++ -std=c++17 -O2 -I monoforce_amd/csrc tools/stream_ring_model.cpp
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
};
struct Op { int kind, arg; };

struct Config { int n_steps, slots, batch; bool handoff; };

// The programs, in the kernel's own order of operations.
static std::vector<Op> fetcher_program(const Config& c, int fk) {
  std::vector<Op> p;
  auto put = [&](int o) {
    p.push_back({F_ROOM, o});
    if (c.handoff) p.push_back({F_TAKE, o});
    p.push_back({F_WRITE, o});
    p.push_back({F_PUBTRY, o + 1});
  };
  const int n_full = c.n_steps / c.batch;
  for (int j = fk; j < n_full; j += 2) {
    p.push_back({F_BATCH, j * c.batch});
    for (int i = 0; i < c.batch; ++i) put(j * c.batch + i);
    p.push_back({F_PUBWAIT, (j + 1) * c.batch});
  }
  if (fk == (n_full & 1))
    for (int o = n_full * c.batch; o < c.n_steps; ++o) { p.push_back({F_BATCH, o}); put(o); p.push_back({F_PUBWAIT, o + 1}); }
  if (fk == 1) p.push_back({F_SNAP, 0});
  if (c.handoff) {
    p.push_back({F_ALLDONE, 0});
    for (int o = sr::first_undrained(c.n_steps, c.slots); o < c.n_steps; ++o)
      if (sr::owner_of(o, c.batch) == fk) p.push_back({F_DRAIN, o});
  }
  return p;
}
static std::vector<Op> computer_program(const Config& c) {
  std::vector<Op> p;
  int consumed = 0;
  auto grab = [&]() { p.push_back({C_GRAB, consumed}); ++consumed; };
  auto finish = [&](int n) {      // the chain of step n is done (ordinal n_steps - 1 - n)
    if (c.handoff) p.push_back({C_ANSWER, c.n_steps - 1 - n});
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
  p.push_back({C_SNAPWAIT, 0});
  return p;
}

constexpr int kMaxSlots = 12;
struct State {
  uint16_t pc[3];                 // fetching wave 0, fetching wave 1, computing wave
  int8_t published, answered, snap, consumed;
  int8_t pub[2];                  // a fetching wave's first written-but-unpublished ordinal
  int8_t ord[kMaxSlots];          // the ordinal a slot holds (-1: its initial contents)
  int8_t st[kMaxSlots];           // 0 written, 1 read by the computing wave, 2 answered, 3 answer consumed
};
static std::string key(const State& s) { return std::string(reinterpret_cast<const char*>(&s), sizeof(State)); }

struct Result { long states = 0; int findings = 0; };

static void finding(Result& r, const Config& c, const char* what, int o) {
  if (r.findings < 20)
    std::printf("FINDING n_steps %d slots %d batch %d %s: %s (ordinal %d)\n", c.n_steps, c.slots, c.batch, c.handoff ? "hand-off" : "read-counted", what, o);
  ++r.findings;
}

static Result explore(const Config& c) {
  Result res;
  const std::vector<Op> prog[3] = {fetcher_program(c, 0), fetcher_program(c, 1), computer_program(c)};
  State s0;
  std::memset(&s0, 0, sizeof(s0));
  for (int i = 0; i < kMaxSlots; ++i) { s0.ord[i] = -1; s0.st[i] = 3; }
  std::unordered_set<std::string> seen;
  std::deque<State> todo;
  seen.insert(key(s0)); todo.push_back(s0);
  while (!todo.empty()) {
    const State s = todo.front(); todo.pop_front();
    ++res.states;
    bool all_done = true, moved = false;
    for (int w = 0; w < 3; ++w) {
      if (s.pc[w] >= prog[w].size()) continue;
      all_done = false;
      const Op op = prog[w][s.pc[w]];
      State t = s;
      bool blocked = false;
      const int sl = op.arg >= 0 ? sr::slot_of(op.arg, c.slots) : 0;
      switch (op.kind) {
        case F_BATCH: t.pub[w] = (int8_t)op.arg; break;
        case F_ROOM: blocked = !sr::has_room(op.arg, s.answered, c.slots); break;
        case F_TAKE: {
          const int old = sr::answer_in_slot(op.arg, c.slots);
          if (old >= 0) {
            if (sr::owner_of(old, c.batch) != w) finding(res, c, "an answer read by the wave that did not write the step", old);
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
    }
    if (res.findings > 100) break;
  }
  return res;
}

int main() {
  static_assert(sr::fixed_ownership(12, 3) && sr::fixed_ownership(6, 3) && !sr::fixed_ownership(6, 2), "ring ownership");
  static_assert(sr::slot_of(13, 12) == 1 && sr::owner_of(5, 3) == 1 && sr::owner_of(6, 3) == 0 && sr::has_room(11, 0, 12) && !sr::has_room(12, 0, 12), "ring arithmetic");
  const struct { int slots, batch; bool handoff; } rings[] = {{12, 3, true}, {6, 3, true}, {12, 3, false}, {6, 3, false}, {6, 2, false}};
  long states = 0;
  int findings = 0;
  for (const auto& r : rings)
    for (int n = 1; n <= 30; ++n) {
      const Result x = explore(Config{n, r.slots, r.batch, r.handoff});
      states += x.states; findings += x.findings;
    }
  if (findings) { std::printf("%d findings\n", findings); return 1; }
  std::printf("explored %ld states\n", states);
  return 0;
}
