// Host side of the persistent per-event scorer (kernels/ae_serve.hip).
//
// Request slots, result slots and the control block are fine-grained pinned host
// memory mapped into the GPU's address space, so an event travels host -> GPU ->
// host with no hipMemcpy and no kernel launch.  Slots are LL-framed (sml_ops.h):
// submit() writes each row as tagged 8-byte words and then publishes the new head;
// the resident wave polls the next slot's words directly; wait() polls the tagged
// result words in host memory.  `done` is only a back-pressure / restart hint.  If
// the kernel exited (idle timeout or a race with its exit), wait() relaunches it; it
// resumes at `done`.
//
// A ring may have several LANES (the wide LSTM forecaster): lane i has its own control block,
// request ring and result ring (ctl_[i], req_ / res_ + i * nslots, one allocation each) and
// its own sequence numbers; one launch on the one persistent stream runs a workgroup per
// lane.  infer() sends key k to lane k % lanes (sml_serve_shard.h) and gathers the results
// back into batch order.  stop and the leave latch are lane 0's words and act on every lane.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

#include "sml_ops.h"

namespace sml {

// A device allocation that frees itself (move-only).
class DeviceBuffer {
 public:
  DeviceBuffer() = default;
  // bytes on the current device, filled from host unless it is null; what: names it in an error
  DeviceBuffer(size_t bytes, const void* host, const char* what);
  ~DeviceBuffer();
  DeviceBuffer(DeviceBuffer&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
  DeviceBuffer& operator=(DeviceBuffer&& o) noexcept;
  template <class T>
  T* as() const { return static_cast<T*>(p_); }

 private:
  void* p_ = nullptr;
};

// The Dense scorers' stats block: 128 host-mapped, coherent bytes whose first word the kernel stores
// after each pass, {passes << 32 | events}, cumulative.
class ServeStats {
 public:
  ServeStats();
  ~ServeStats();
  ServeStats(const ServeStats&) = delete;
  ServeStats& operator=(const ServeStats&) = delete;
  uint64_t* device() const { return dev_; }
  // the word, read once it covers `events` events (bounded wait: the kernel stores it a moment after
  // the result words that the host polls)
  uint64_t read(uint64_t events) const;

 private:
  uint64_t* host_ = nullptr;
  uint64_t* dev_ = nullptr;
};

// The host-mapped request / result rings and the relaunch-on-demand protocol shared by the
// persistent scorers; a subclass supplies the kernel launch.
class ServeRing {
 public:
  // max_D: widest row the subclass's kernel takes (<= 32 request words; 31 when word 31
  // carries a key)
  // nslots: slots per lane
  ServeRing(int device, int nslots, int D, double idle_seconds, int max_D, int lanes = 1);
  virtual ~ServeRing();
  ServeRing(const ServeRing&) = delete;
  ServeRing& operator=(const ServeRing&) = delete;

  // Publish k rows of D floats to one lane (keys: optional per-row uint32 in request word
  // 31); returns the lane's sequence number of the first one.
  uint64_t submit(const float* rows, int k, const uint32_t* keys = nullptr, int lane = 0);
  // Block until the results of the lane's events in [seq_end - nslots, seq_end) have landed
  // (throws after timeout_s).
  void wait(uint64_t seq_end, double timeout_s, int lane = 0);
  const ServeResult& result(uint64_t seq, int lane = 0) const { return slot_res(seq, lane); }
  // all tagged words of event seq's result have landed
  bool complete(uint64_t seq, int lane = 0) const;
  // payload of result word i of event seq (call after complete())
  uint32_t word(uint64_t seq, int i, int lane = 0) const;
  float score(uint64_t seq, int lane = 0) const;
  // submit + wait + copy scores / flags (/ recon) for k rows.  With several lanes (keys
  // required) each row goes to its key's lane, in batch order within the lane; back-pressure
  // is per lane: when a lane's ring is full the host gathers that lane's oldest results
  // (the other lanes keep draining on the device) before it publishes more.
  void infer(const float* rows, int k, float* scores, uint32_t* flags, float* recon, double timeout_s,
             const uint32_t* keys = nullptr);
  // Per-event latency (ns) of n events submitted one at a time, spaced by gap_ns.
  // Also fills dev_ns[i] (device pick-up -> stores issued, if non-null) and counts relaunches.
  std::vector<int64_t> latency_run(const float* rows, int n, int64_t gap_ns, std::vector<int64_t>* dev_ns = nullptr,
                                   const uint32_t* keys = nullptr);
  void stop();
  int D() const { return D_; }
  int lanes() const { return lanes_; }
  int nslots() const { return nslots_; }
  // debugging: {head, done, stop, alive, launches, stream idle (1) / busy (0)} of a lane, then
  // the raw result words and request words of its event `seq`'s slot
  std::vector<uint64_t> debug_state(uint64_t seq, int lane = 0) const;
  uint64_t launches() const { return launches_; }
  // events each lane completed since construction or mark_lane_events(), from the lanes'
  // completion counters
  std::vector<int64_t> lane_events() const;

 protected:
  virtual hipError_t launch_kernel() = 0;
  void launch();
  // back-pressure: block until the device consumed every event < n (its request slot is free)
  void wait_done(uint64_t n, double timeout_s, int lane = 0);
  void mark_lane_events();   // lane_events() counts from here
  // stop the resident kernel and wait until it has left (alive == 0): what a copy into memory the
  // kernel reads needs, so that it never queues behind a kernel that only leaves at its idle timeout
  void halt();
  // the optional input normaliser: both empty, or D entries each (else invalid_argument "<who>:
  // scale/shift size"); upload_affine fills scale_d_ / shift_d_
  static void check_affine(const std::vector<float>& scale, const std::vector<float>& shift, int D, const char* who);
  void upload_affine(const std::vector<float>& scale, const std::vector<float>& shift, const char* who);
  // the front both Dense scorers' argument structs share (rings, D, layer table, normaliser, idle
  // ticks, stats word); the structs stay two: their layout is part of the kernels
  template <class Args>
  void fill_dense_args(Args& a, const std::vector<DenseServeLayer>& layers, const ServeStats& stats) const;
  int device_, nslots_, D_, lanes_;
  double idle_s_;
  ServeCtl* ctl_ = nullptr;      // [lanes]
  ServeReq* req_ = nullptr;      // [lanes][nslots]
  ServeResult* res_ = nullptr;   // [lanes][nslots]
  ServeCtl* ctl_d_ = nullptr;
  ServeReq* req_d_ = nullptr;
  ServeResult* res_d_ = nullptr;
  hipStream_t stream_ = nullptr;
  DeviceBuffer scale_d_, shift_d_;   // [D] each, or empty
  std::vector<uint64_t> head_;       // per lane: events published
  std::vector<uint64_t> complete_;   // per lane: events known complete (prefix)
  std::vector<uint64_t> done0_;      // per lane: `done` at mark_lane_events()
  uint64_t launches_ = 0;
  const char* name_ = "serve";

 private:
  ServeReq& slot_req(uint64_t seq, int lane) const {
    return req_[(size_t)lane * (size_t)nslots_ + (size_t)(seq % (uint64_t)nslots_)];
  }
  ServeResult& slot_res(uint64_t seq, int lane) const {
    return res_[(size_t)lane * (size_t)nslots_ + (size_t)(seq % (uint64_t)nslots_)];
  }
  void copy_result(uint64_t seq, int lane, int row, float* scores, uint32_t* flags, float* recon) const;
  void infer_lanes(const float* rows, int k, float* scores, uint32_t* flags, float* recon, double timeout_s,
                   const uint32_t* keys);
};

// Dense autoencoder scorer (ae_serve.hip): reconstruction + MSE anomaly score per event.
class AEServe : public ServeRing {
 public:
  AEServe(int device, int nslots, const std::vector<float>& weights, const int dims[3], const int acts[4],
          const std::vector<float>& scale, const std::vector<float>& shift, float threshold, double idle_seconds);
  ~AEServe() override { stop(); }   // before any member frees its buffer

 protected:
  hipError_t launch_kernel() override;

 private:
  int dims_[3], acts_[4];
  float threshold_;
  DeviceBuffer wts_d_;
};

// Dense stacks of any depth (dense_serve.hip): 1..8 Dense layers up to 512 wide, rows of up to
// 32 features, the last layer one unit per feature; one lane, up to DSV_EB events per pass.
class DenseServe : public ServeRing {
 public:
  // image: the packed weight image (ops/serve.py dense_serve_image; sml_ops.h), layers: its table
  DenseServe(int device, int nslots, const std::vector<float>& image, const std::vector<DenseServeLayer>& layers,
             int D, const std::vector<float>& scale, const std::vector<float>& shift, float threshold,
             double idle_seconds);
  ~DenseServe() override { stop(); }   // before any member frees its buffer
  // where the resident kernel keeps the image: "lds" | "stream"
  const char* kernel() const { return in_lds_ ? "lds" : "stream"; }
  // passes the kernel ran and events they served since construction (its stats word, read once
  // it covers every event this host has gathered)
  uint64_t passes() const { return stats_.read(complete_[0]) >> 32; }
  uint64_t events() const { return stats_.read(complete_[0]) & 0xffffffffull; }

 protected:
  hipError_t launch_kernel() override;

 private:
  // every limit, before the base class allocates the rings; returns D
  static int checked_D(const std::vector<float>& image, const std::vector<DenseServeLayer>& layers, int D,
                       const std::vector<float>& scale, const std::vector<float>& shift);
  DenseServeArgs args_{};
  bool in_lds_ = false;
  ServeStats stats_;
  DeviceBuffer img_d_;
};

// A fleet of Dense stacks of one shape (dense_serve_fleet.hip): every event names the model that
// scores it (request word 31), so rows have up to 31 features; one lane, up to DSV_EB events per
// pass.  The server owns the stacked images, the per-model thresholds and the stats block.
class DenseFleetServe : public ServeRing {
 public:
  // images: n_models images of `stride` floats each, one after the other (ops/serve.py
  // dense_fleet_serve_images); layers: the one table, offsets relative to a model's image;
  // thresholds: one per model
  DenseFleetServe(int device, int nslots, const float* images, int64_t n_models, int64_t stride, int64_t img_floats,
                  const std::vector<DenseServeLayer>& layers, int D, const std::vector<float>& scale,
                  const std::vector<float>& shift, const std::vector<float>& thresholds, double idle_seconds);
  ~DenseFleetServe() override { stop(); }   // before any member frees its buffer
  int64_t n_models() const { return args_.n_models; }
  int64_t stride() const { return args_.stride; }
  const char* kernel() const { return "fleet"; }
  uint64_t passes() const { return stats_.read(complete_[0]) >> 32; }
  uint64_t events() const { return stats_.read(complete_[0]) & 0xffffffffull; }
  // submit + wait + copy for k rows, row i scored by model models[i].  Every index is checked
  // before anything is published: std::invalid_argument names the first one >= n_models.
  void infer(const float* rows, const uint32_t* models, int k, float* scores, uint32_t* flags, float* recon,
             double timeout_s);
  // the first index >= n_models among models[0 .. k), or -1
  int64_t first_bad_index(const uint32_t* models, int64_t k) const;
  // Replace model i's image (stride floats) / the whole stack (n_models * stride floats): stops the
  // resident kernel and waits until it has left (alive == 0), copies; the next submit relaunches.
  void set_image(int64_t i, const float* image);
  void set_images(const float* images);

 protected:
  hipError_t launch_kernel() override;

 private:
  static int checked_D(const float* images, int64_t n_models, int64_t stride, int64_t img_floats,
                       const std::vector<DenseServeLayer>& layers, int D, const std::vector<float>& scale,
                       const std::vector<float>& shift, const std::vector<float>& thresholds);
  DenseFleetServeArgs args_{};
  ServeStats stats_;
  DeviceBuffer img_d_, thr_d_;
};

// LSTM forecaster (lstm_serve.hip): per car key, the last T events stay on the device; each
// event is scored against the key's previous forecast and a new forecast is emitted.
class LSTMServe : public ServeRing {
 public:
  // layers: LstmServeLayer descriptors (offsets into weights); keys in [0, nkeys); lanes:
  // resident workgroups (1..LSW_MAXLANES, at most half the device's CUs; more than one only
  // for stacks that take the wide kernel), key k is served by lane k % lanes
  LSTMServe(int device, int nslots, const std::vector<float>& weights, const std::vector<LstmServeLayer>& layers,
            int D, int T, int nkeys, const std::vector<float>& scale, const std::vector<float>& shift, float threshold,
            double idle_seconds, int lanes = 1);
  ~LSTMServe() override { stop(); }   // before any member frees its buffer
  int nkeys() const { return args_.nkeys; }
  // forget every key's window and forecast: stops the resident kernel, zeroes the key state
  // on the device, relaunches (returns without waiting for the kernel's idle timeout)
  void reset_keys();
  // the kernel lstm_serve_launch chose for this stack: "ref1" | "pipe" | "generic" | "wide"
  const char* kernel() const;

 protected:
  hipError_t launch_kernel() override;

 private:
  // every limit on `lanes`, before the base class allocates the rings; returns lanes
  static int checked_lanes(int device, int lanes, const std::vector<LstmServeLayer>& layers, int D, int T);
  // wide stacks: bf16 images of every LSTM layer's W and U, padded biases (one allocation)
  // and each lane's input projection scratch, built once before the resident kernel starts
  void build_wide(const std::vector<float>& weights);
  LstmServeArgs args_{};
  int kernel_ = LSK_GENERIC;
  DeviceBuffer wts_d_, wide_d_, wide_zx_d_;
  DeviceBuffer hist_d_, hcount_d_, lastpred_d_;   // the key state
};

}  // namespace sml
