// map_product.hpp -- what the products of an int8 map (clearance.hip, frontier.hip, route.hip, view.hip) share on the host: where a
// call's map comes from and which stream the call runs on (the rule itself: map_source_rule.hpp), and the kept scratch buffers that
// grow on demand.
#pragma once
#include "capi_internal.hpp"
#include "map_source_rule.hpp"

namespace tsd {

// The map of a call and the stream it runs on.  timed: the passes show in the context's kernel profile (the context's stream only).
struct MapSource { MapView m; hipStream_t stream; bool timed; };

// a refusal in the name of the entry point `who`
inline int map_refused(tsd_ctx* ctx, const char* who, const char* why) { return set_error(ctx, TSD_E_ARG, (std::string(who) + ": " + why).c_str(), hipSuccess); }

// A map of the caller's in device memory, read on the context's stream.  Enqueues nothing.
inline int map_source_caller(tsd_ctx* ctx, const char* who, const void* map_dev, int width, int height, int stride, MapSource* src)
{
  if (const char* why = caller_map_wrong(map_dev, width, height, stride, TSD_FRONTIER_MAX_SIDE)) return map_refused(ctx, who, why);
  *src = MapSource{MapView{static_cast<const int8_t*>(map_dev), width, height, (size_t)stride}, ctx->stream, true};
  return TSD_OK;
}

// The staged map of the last published frame (want_cost: the cost map made of it), read on the copy stream.  Enqueues nothing.
inline int map_source_frame(tsd_ctx* ctx, const char* who, bool want_cost, MapSource* src, int max_side = TSD_FRONTIER_MAX_SIDE)
{
  const int8_t* staged = frame_staged_map(ctx);
  const int N = ctx->grid.N;
  const FrameState s{ctx->clearance.inflight, ctx->frame_inflight, ctx->frame_map_valid, staged != nullptr, N,
                     ctx->clearance.d_cost != nullptr, ctx->clearance.cost_cells};
  if (const char* why = frame_map_wrong(s, max_side, want_cost)) return map_refused(ctx, who, why);
  *src = MapSource{MapView{want_cost ? ctx->clearance.d_cost : staged, N, N, (size_t)N}, ctx->stream_io, false};
  return TSD_OK;
}

// The top of a call once its arguments stand: the device, and the stream behind what it has to follow.
inline int map_source_enter(tsd_ctx* ctx, const MapSource& src)
{
  if (src.stream == ctx->stream) return enter(ctx);
  TSD_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  // On the copy stream, behind the frame's kernels (a cost map's ran there and were waited for): the grid's stream never waits for a map product.
  TSD_HIP_CHECK(ctx, hipStreamWaitEvent(ctx->stream_io, ctx->ev_frame, 0));
  return TSD_OK;
}

// p (capacity *cap elements) holds `need` elements, or TSD_E_NOMEM "<who>: the device cannot hold <what> (<bytes> bytes)" with p null
// and *cap 0.  The old buffer is freed first: nothing of the context reads it, every call of these products has waited for its own
// work.  pinned: page-locked host memory.  What a product's result loses with its scratch is the caller's to say.
template <typename T>
int scratch_grow(tsd_ctx* ctx, const char* who, T** p, size_t* cap, size_t need, const char* what, bool pinned = false)
{
  if (*cap >= need) return TSD_OK;
  if (*p) { if (pinned) hipHostFree(*p); else hipFree(*p); }
  *p = nullptr; *cap = 0;
  const size_t bytes = need * sizeof(T);
  const hipError_t e = pinned ? hipHostMalloc(reinterpret_cast<void**>(p), bytes, hipHostMallocDefault) : hipMalloc(reinterpret_cast<void**>(p), bytes);
  if (e != hipSuccess) *p = nullptr;
  if (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation) {
    (void)hipGetLastError();
    char buf[160];
    snprintf(buf, sizeof(buf), "%s: the device cannot hold %s (%zu bytes)", who, what, bytes);
    return set_error(ctx, TSD_E_NOMEM, buf, hipSuccess);
  }
  if (e != hipSuccess) return set_error(ctx, TSD_E_HIP, (std::string("allocation (") + who + ")").c_str(), e);
  *cap = need;
  return TSD_OK;
}

// Several buffers under one capacity, each of `per` elements per unit of it: where *cap < need every one of them is replaced, and
// *cap is 0 unless all of them stand.
template <typename T> struct ScratchPart { T** p; const char* what; bool pinned; size_t per; };
template <typename T> ScratchPart<T> scratch_part(T** p, const char* what, bool pinned = false, size_t per = 1) { return ScratchPart<T>{p, what, pinned, per}; }

template <typename... Ts>
int scratch_grow_all(tsd_ctx* ctx, const char* who, size_t* cap, size_t need, ScratchPart<Ts>... parts)
{
  if (*cap >= need) return TSD_OK;
  *cap = 0;
  int rc = TSD_OK;
  auto one = [&](auto part) { size_t none = 0; rc = scratch_grow(ctx, who, part.p, &none, need * part.per, part.what, part.pinned); return rc == TSD_OK; };
  if ((one(parts) && ...)) *cap = need;                // (the first failure ends the row)
  return rc;
}

}  // namespace tsd
