// grid_ledger.hpp -- what the host remembers about the writes to one grid: which ray casts they outdate, which tiles the next push
// and the next windowed map frame have to cover.  Plain host arithmetic, no HIP: tests/grid_ledger_check.cpp runs it on the CPU.
#pragma once

namespace tsd {

// inclusive tile rectangle (empty when x1 < x0)
struct TileBox {
  int x0 = 0, y0 = 0, x1 = -1, y1 = -1;
  bool empty() const { return x1 < x0 || y1 < y0; }
  void add(const TileBox& o)
  {
    if (o.empty()) return;
    if (empty()) { *this = o; return; }
    if (o.x0 < x0) x0 = o.x0; if (o.y0 < y0) y0 = o.y0; if (o.x1 > x1) x1 = o.x1; if (o.y1 > y1) y1 = o.y1;
  }
};

// Every entry point that changes the grid, a sensor pose or the context's ray-cast outputs reports it here, by the name of what it
// did; nothing else writes these fields.  Who may call, under which lock: see tsd_ctx::ledger.
class GridLedger {
 public:
  // ---- the epoch: only ever compared for equality.  The fused scan enqueues the NEXT scan's ray cast behind its push and remembers
  // the epoch; that ray cast stands for the next scan only if nothing below happened in between (tsd_scan_submit).
  unsigned long long epoch() const { return epoch_; }
  // the context's ray-cast outputs or a sensor's pose were overwritten (tsd_raycast, tsd_icp*, tsd_localize, tsd_relocalize,
  // tsd_sensor_set_pose): the grid itself is as it was
  void outputs_overwritten() { epoch_++; }
  // A push whose own tile window is `cur` (launch_push, launch_push_multi): the window to launch also covers the previous push (its
  // tile records are rewritten) and whatever a footprint touched since.  Counted whether or not a device-side gate lets the push run.
  TileBox push_window(const TileBox& cur)
  {
    TileBox box = cur;
    box.add(prev_); box.add(dirty_);
    prev_ = cur; dirty_ = TileBox{};
    frame_.add(box); epoch_++;
    return box;
  }
  // freeFootprint wrote the tiles of `b` (launch_free_footprint): the next push refreshes the halos there, the next windowed frame
  // covers them
  void footprint(const TileBox& b) { dirty_.add(b); frame_.add(b); epoch_++; }
  // The grid was rewritten wholesale: the next tsd_map_update_begin takes a full frame.  As it stands (tsd_set_max_truncation) ...
  void grid_rewritten() { frame_prev_valid_ = false; epoch_++; }
  // ... with the push bookkeeping cleared along with it (reset_push_bookkeeping: tsd_reset, the destination of tsd_fuse_begin) ...
  void grid_reset() { prev_ = TileBox{}; dirty_ = TileBox{}; grid_rewritten(); }
  // ... or from tiles whose halos came as given (tsd_upload_tiles): the next push refreshes them all over the grid, `all`
  void grid_uploaded(const TileBox& all) { dirty_.add(all); grid_rewritten(); }
  // ---- the windowed map frame (tsd_map_update_begin); none of this moves the epoch.
  // The tiles anything may have written since the last frame was enqueued: every push's launch window, every footprint.
  const TileBox& frame_box() const { return frame_; }
  // May the next frame be the window around frame_box()?  Only where the staging holds a complete frame of the same parameters (and
  // its image, if one is wanted) of the grid as frame_box() describes it.  (With factor > 31 a mark at u + factor > N spills into
  // the next row, far from any window: DESIGN 3.4.)
  bool frame_may_be_windowed(bool image, int inflate, int factor) const
  {
    return frame_prev_valid_ && (!image || frame_prev_image_) && frame_prev_inflate_ == inflate &&
           (!inflate || (frame_prev_factor_ == factor && factor >= 0 && factor <= 31));
  }
  // a frame is being enqueued: until it is out completely the staging holds no frame to build on
  void frame_started() { frame_prev_valid_ = false; }
  void frame_enqueued(bool image, int inflate, int factor)
  {
    frame_ = TileBox{};
    frame_prev_valid_ = true; frame_prev_image_ = image; frame_prev_inflate_ = inflate; frame_prev_factor_ = factor;
  }
  // the staging was replaced, or a frame ended in an error: frame_box() stays, the next frame is a full one
  void frame_lost() { frame_prev_valid_ = false; }
 private:
  unsigned long long epoch_ = 0;
  TileBox prev_{}, dirty_{}, frame_{};   // what the last push covered, what freeFootprint dirtied since; frame_: see frame_box()
  bool frame_prev_valid_ = false, frame_prev_image_ = false;
  int frame_prev_inflate_ = 0, frame_prev_factor_ = 0;
};

}  // namespace tsd
