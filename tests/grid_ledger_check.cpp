// grid_ledger_check.cpp -- tsd::GridLedger (csrc/grid_ledger.hpp) on the CPU: tables of calls with what each must return and leave,
// written out by hand from DESIGN 1 / 3.4 (launch window = current + previous push + footprints since; frame box = every launch window
// and footprint since the last enqueued frame; when an update may be windowed; what moves the epoch).  Built and run by
// tests/test_cpu_grid_ledger.py under -fsanitize=address,undefined.  Prints "ok <case>" per table, "grid_ledger: all cases ok" at the end.
#include "grid_ledger.hpp"

#include <cstdio>
#include <vector>

using tsd::GridLedger;
using tsd::TileBox;

static TileBox box(int x0, int y0, int x1, int y1) { TileBox b; b.x0 = x0; b.y0 = y0; b.x1 = x1; b.y1 = y1; return b; }
static bool same(const TileBox& a, const TileBox& b)
{
  if (a.empty() || b.empty()) return a.empty() && b.empty();
  return a.x0 == b.x0 && a.y0 == b.y0 && a.x1 == b.x1 && a.y1 == b.y1;
}

static const TileBox NONE{};                       // the empty box
static const TileBox A = box(2, 2, 4, 4), B = box(6, 3, 8, 5), C = box(10, 1, 12, 3);
static const TileBox AB = box(2, 2, 8, 5), BC = box(6, 1, 12, 5);
static const TileBox F = box(20, 20, 21, 21);      // a footprint away from all of them
static const TileBox ABF = box(2, 2, 21, 21), AF = box(2, 2, 21, 21);
static const TileBox ALL = box(0, 0, 31, 31);      // every tile of a 1024^2 grid

enum Op {
  PUSH, FOOTPRINT, OUTPUTS, REWRITTEN, RESET, UPLOAD,          // these move the epoch
  MAY_WINDOW, STARTED, ENQUEUED, LOST                          // these do not
};

struct Step {
  Op op;
  TileBox arg;                   // PUSH: the push's own window; FOOTPRINT: its box; UPLOAD: all tiles
  bool image; int inflate, factor;                             // MAY_WINDOW, ENQUEUED
  TileBox want_window;           // PUSH: the launch window returned
  int want_may;                  // MAY_WINDOW: 1 windowed, 0 full frame
  TileBox want_frame;            // the frame box AFTER the step
  const char* what;
};

static Step push(const TileBox& cur, const TileBox& window, const TileBox& frame, const char* what) { return Step{PUSH, cur, false, 0, 0, window, -1, frame, what}; }
static Step foot(const TileBox& b, const TileBox& frame, const char* what) { return Step{FOOTPRINT, b, false, 0, 0, NONE, -1, frame, what}; }
static Step plain(Op op, const TileBox& frame, const char* what) { return Step{op, NONE, false, 0, 0, NONE, -1, frame, what}; }
static Step upload(const TileBox& frame, const char* what) { return Step{UPLOAD, ALL, false, 0, 0, NONE, -1, frame, what}; }
static Step may(bool image, int inflate, int factor, int want, const TileBox& frame, const char* what) { return Step{MAY_WINDOW, NONE, image, inflate, factor, NONE, want, frame, what}; }
static Step enq(bool image, int inflate, int factor, const char* what) { return Step{ENQUEUED, NONE, image, inflate, factor, NONE, -1, NONE, what}; }

static int failures = 0;

static void run(const char* name, const std::vector<Step>& steps)
{
  GridLedger l;
  int bad = 0;
  auto fail = [&](size_t i, const char* msg) { std::printf("FAIL %s step %zu (%s): %s\n", name, i, steps[i].what, msg); bad++; };
  for (size_t i = 0; i < steps.size(); i++) {
    const Step& s = steps[i];
    const unsigned long long e0 = l.epoch();
    switch (s.op) {
      case PUSH: {
        const TileBox w = l.push_window(s.arg);
        if (!same(w, s.want_window)) { std::printf("  got window %d %d %d %d\n", w.x0, w.y0, w.x1, w.y1); fail(i, "launch window"); }
        break;
      }
      case FOOTPRINT: l.footprint(s.arg); break;
      case OUTPUTS: l.outputs_overwritten(); break;
      case REWRITTEN: l.grid_rewritten(); break;
      case RESET: l.grid_reset(); break;
      case UPLOAD: l.grid_uploaded(s.arg); break;
      case MAY_WINDOW:
        if ((int)l.frame_may_be_windowed(s.image, s.inflate, s.factor) != s.want_may) fail(i, "windowed / full decision");
        break;
      case STARTED: l.frame_started(); break;
      case ENQUEUED: l.frame_enqueued(s.image, s.inflate, s.factor); break;
      case LOST: l.frame_lost(); break;
    }
    const bool moves = s.op <= UPLOAD;
    if (moves && !(l.epoch() > e0)) fail(i, "the epoch did not rise");
    if (!moves && l.epoch() != e0) fail(i, "the epoch moved");
    if (!same(l.frame_box(), s.want_frame)) {
      const TileBox& f = l.frame_box();
      std::printf("  got frame box %d %d %d %d\n", f.x0, f.y0, f.x1, f.y1);
      fail(i, "frame box");
    }
  }
  if (bad) failures += bad; else std::printf("ok %s\n", name);
}

int main()
{
  // a fresh ledger: epoch 0, nothing to cover, no frame to build on
  {
    GridLedger l;
    if (l.epoch() != 0 || !l.frame_box().empty() || l.frame_may_be_windowed(false, 0, 0)) { std::printf("FAIL fresh ledger\n"); failures++; }
    else std::printf("ok fresh_ledger\n");
  }

  run("windows_of_three_pushes", {
    push(A, A, A, "push A"),
    push(B, AB, AB, "push B covers A"),
    push(C, BC, box(2, 1, 12, 5), "push C covers B, not A"),
  });

  run("footprint_widens_the_next_window_once", {
    push(A, A, A, "push A"),
    foot(F, AF, "footprint"),
    push(B, ABF, ABF, "push B covers A and the footprint"),
    push(C, BC, box(2, 1, 21, 21), "push C covers B only"),
    foot(NONE, box(2, 1, 21, 21), "an empty footprint counts and covers nothing"),
    push(A, box(2, 1, 12, 4), box(2, 1, 21, 21), "push A covers C only"),
  });

  run("frame_box_is_everything_since_the_last_enqueued_frame", {
    push(A, A, A, "push A"),
    foot(F, AF, "footprint"),
    push(B, ABF, ABF, "push B"),
    plain(OUTPUTS, ABF, "a ray cast's outputs overwritten"),
    plain(STARTED, ABF, "frame started"),
    enq(true, 1, 2, "frame enqueued: the box starts over"),
    push(C, BC, BC, "push C: its launch window, previous push included"),
    foot(F, box(6, 1, 21, 21), "footprint"),
    enq(true, 1, 2, "frame enqueued"),
    foot(F, F, "a footprint alone"),
  });

  run("frame_box_survives_a_lost_frame", {
    push(A, A, A, "push A"),
    plain(STARTED, A, "first frame started"),
    enq(false, 0, 0, "first frame enqueued"),
    push(B, AB, AB, "push B"),
    may(false, 0, 0, 1, AB, "an update may be windowed"),
    plain(STARTED, AB, "update started"),
    plain(LOST, AB, "... and lost"),
    may(false, 0, 0, 0, AB, "the next one is a full frame"),
    push(C, BC, box(2, 1, 12, 5), "push C adds to the box that was kept"),
  });

  run("wholesale_rewrites", {
    push(A, A, A, "push A"),
    enq(false, 1, 2, "frame enqueued"),
    plain(REWRITTEN, NONE, "set_max_truncation: nothing but the frame's validity"),
    may(false, 1, 2, 0, NONE, "full frame after it"),
    push(B, AB, AB, "push B still covers A"),
    plain(RESET, AB, "reset forgets the pushes"),
    push(C, C, box(2, 1, 12, 5), "push C alone"),
    upload(box(2, 1, 12, 5), "upload marks every tile dirty, the frame box is not its business"),
    push(A, ALL, ALL, "the push after an upload covers the grid"),
    push(B, AB, ALL, "the one after it does not"),
  });

  // tests/test_gpu_map_update.py::test_fallbacks_return_the_whole_map, the same calls at the ledger's level: a map update asks,
  // starts and enqueues; P is a push's own window
  const TileBox P = box(12, 2, 17, 7);
  auto update = [](std::vector<Step>& v, bool image, int inflate, int factor, int want, const TileBox& frame, const char* what) {
    v.push_back(may(image, inflate, factor, want, frame, what));
    v.push_back(plain(STARTED, frame, what));
    v.push_back(enq(image, inflate, factor, what));
  };
  {
    std::vector<Step> v;
    v.push_back(push(P, P, P, "first push"));
    update(v, true, 1, 2, 0, P, "first call");
    v.push_back(push(P, P, P, "push"));
    update(v, true, 1, 2, 1, P, "second call, same parameters");
    update(v, true, 1, 3, 0, NONE, "changed factor");
    v.push_back(push(P, P, P, "push"));
    update(v, true, 1, 3, 1, P, "same factor again");
    update(v, true, 0, 3, 0, NONE, "inflation off");
    v.push_back(may(true, 0, 7, 1, NONE, "(without inflation the factor does not matter)"));
    update(v, true, 1, 32, 0, NONE, "factor 32");
    v.push_back(push(P, P, P, "push"));
    update(v, true, 1, 32, 0, P, "factor 32 again");
    update(v, true, 1, 3, 0, NONE, "back to factor 3");
    v.push_back(plain(RESET, NONE, "tsd_reset"));
    update(v, true, 1, 3, 0, NONE, "after tsd_reset");
    v.push_back(push(P, P, P, "push"));
    update(v, true, 1, 3, 1, P, "after the reset's frame");
    v.push_back(upload(NONE, "tsd_upload_tiles"));
    update(v, true, 1, 3, 0, NONE, "after tsd_upload_tiles (the box was empty)");
    v.push_back(plain(RESET, NONE, "fuse destination"));
    update(v, true, 1, 3, 0, NONE, "after fuse_from");
    v.push_back(may(true, 1, 3, 1, NONE, "... and windowed (and empty) after that"));
    v.push_back(may(true, 1, -1, 0, NONE, "(a negative factor is never windowed)"));
    run("fallbacks_return_the_whole_map", v);
  }
  {
    std::vector<Step> v;
    v.push_back(push(P, P, P, "first push"));
    update(v, false, 1, 2, 0, P, "map-only, first call");
    v.push_back(push(P, P, P, "push"));
    update(v, false, 1, 2, 1, P, "map-only update");
    v.push_back(push(P, P, P, "push"));
    update(v, true, 1, 2, 0, P, "image switched on");
    v.push_back(may(false, 1, 2, 1, NONE, "map-only after a frame with an image"));
    run("image_switched_on_after_map_only_frames", v);
  }

  run("epoch_rows", {
    plain(OUTPUTS, NONE, "outputs overwritten"),
    push(A, A, A, "push window"),
    foot(F, AF, "footprint"),
    plain(REWRITTEN, AF, "rewritten as it stands"),
    plain(RESET, AF, "rewritten with the pushes forgotten"),
    upload(AF, "rewritten from uploaded tiles"),
    may(true, 1, 2, 0, AF, "asking"),
    plain(STARTED, AF, "frame started"),
    plain(LOST, AF, "frame lost"),
    enq(true, 1, 2, "frame enqueued"),
    may(true, 1, 2, 1, NONE, "asking again"),
  });

  if (failures) { std::printf("grid_ledger: %d failures\n", failures); return 1; }
  std::printf("grid_ledger: all cases ok\n");
  return 0;
}
