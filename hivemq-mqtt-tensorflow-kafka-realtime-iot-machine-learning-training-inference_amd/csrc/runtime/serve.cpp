#include "serve.h"
#include "queues.h"
#include "sml_serve_shard.h"

#include <chrono>
#include <cstring>
#include <stdexcept>
#include <string>
#include <thread>
#include <algorithm>

namespace sml {
namespace {

void ck(hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string("serve: ") + what + ": " + hipGetErrorString(e));
}

inline uint64_t load_acq(const uint64_t* p) { return __atomic_load_n(p, __ATOMIC_ACQUIRE); }
inline void store_rel(uint64_t* p, uint64_t v) { __atomic_store_n(p, v, __ATOMIC_RELEASE); }

inline void cpu_relax() {
#if defined(__x86_64__)
  __builtin_ia32_pause();
#endif
}

}  // namespace

DeviceBuffer::DeviceBuffer(size_t bytes, const void* host, const char* what) {
  ck(hipMalloc(&p_, bytes), (std::string("hipMalloc ") + what).c_str());
  if (host) ck(hipMemcpy(p_, host, bytes, hipMemcpyHostToDevice), (std::string("copy ") + what).c_str());
}

DeviceBuffer::~DeviceBuffer() {
  if (p_) (void)hipFree(p_);
}

DeviceBuffer& DeviceBuffer::operator=(DeviceBuffer&& o) noexcept {
  std::swap(p_, o.p_);
  return *this;
}

ServeStats::ServeStats() {
  ck(hipHostMalloc((void**)&host_, 128, hipHostMallocMapped | hipHostMallocCoherent), "hipHostMalloc stats");
  std::memset(host_, 0, 128);
  ck(hipHostGetDevicePointer((void**)&dev_, host_, 0), "device ptr stats");
}

ServeStats::~ServeStats() {
  if (host_) (void)hipHostFree(host_);
}

uint64_t ServeStats::read(uint64_t events) const {
  const uint32_t want = (uint32_t)events;
  const auto t0 = std::chrono::steady_clock::now();
  uint64_t v = load_acq(host_);
  while ((uint32_t)v != want && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() < 0.5) {
    cpu_relax();
    v = load_acq(host_);
  }
  return v;
}

ServeRing::ServeRing(int device, int nslots, int D, double idle_seconds, int max_D, int lanes)
    : device_(device), nslots_(nslots), D_(D), lanes_(lanes), idle_s_(idle_seconds) {
  if (nslots < 64) throw std::invalid_argument("serve: nslots must be >= 64");
  if (lanes < 1 || lanes > LSW_MAXLANES)
    throw std::invalid_argument(std::string("serve: lanes must be 1..") + std::to_string((int)LSW_MAXLANES));
  if (max_D > 32) max_D = 32;   // a request slot holds 32 words
  if (D < 1 || D > max_D)
    throw std::invalid_argument(std::string("serve: rows must have 1..") + std::to_string(max_D) + " features");
  head_.assign((size_t)lanes, 0);
  complete_.assign((size_t)lanes, 0);
  done0_.assign((size_t)lanes, 0);
  ck(hipSetDevice(device), "hipSetDevice");
  const unsigned fl = hipHostMallocMapped | hipHostMallocCoherent;
  const size_t nall = (size_t)nslots * (size_t)lanes;
  ck(hipHostMalloc((void**)&ctl_, sizeof(ServeCtl) * (size_t)lanes, fl), "hipHostMalloc ctl");
  ck(hipHostMalloc((void**)&req_, sizeof(ServeReq) * nall, fl), "hipHostMalloc req");
  ck(hipHostMalloc((void**)&res_, sizeof(ServeResult) * nall, fl), "hipHostMalloc res");
  std::memset(ctl_, 0, sizeof(ServeCtl) * (size_t)lanes);
  std::memset(req_, 0, sizeof(ServeReq) * nall);   // tag 0 = empty (tags start at 1)
  std::memset(res_, 0, sizeof(ServeResult) * nall);
  ck(hipHostGetDevicePointer((void**)&ctl_d_, ctl_, 0), "device ptr ctl");
  ck(hipHostGetDevicePointer((void**)&req_d_, req_, 0), "device ptr req");
  ck(hipHostGetDevicePointer((void**)&res_d_, res_, 0), "device ptr res");
  ck(create_persistent_stream(&stream_), "stream");
}

ServeRing::~ServeRing() {
  if (stream_) (void)hipStreamDestroy(stream_);
  if (ctl_) (void)hipHostFree(ctl_);
  if (req_) (void)hipHostFree(req_);
  if (res_) (void)hipHostFree(res_);
}

void ServeRing::launch() {
  ck(hipSetDevice(device_), "hipSetDevice");
  // only ever called on a drained stream: no lane of an earlier launch can set the latch again
  __atomic_store_n(&ctl_->leave, 0u, __ATOMIC_RELAXED);
  __atomic_store_n(&ctl_->stop, 0u, __ATOMIC_RELEASE);
  ck(launch_kernel(), "launch");
  ++launches_;
}

void ServeRing::halt() {
  stop();
  const auto t0 = std::chrono::steady_clock::now();
  while (__atomic_load_n(&ctl_->alive, __ATOMIC_ACQUIRE) != 0) {   // stored last by the leaving kernel
    cpu_relax();
    if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 10.0)
      throw std::runtime_error(std::string(name_) + ": the resident kernel did not leave");
  }
}

void ServeRing::check_affine(const std::vector<float>& scale, const std::vector<float>& shift, int D, const char* who) {
  if (!scale.empty() && ((int)scale.size() != D || (int)shift.size() != D))
    throw std::invalid_argument(std::string(who) + ": scale/shift size");
}

void ServeRing::upload_affine(const std::vector<float>& scale, const std::vector<float>& shift, const char* who) {
  check_affine(scale, shift, D_, who);
  if (scale.empty()) return;
  scale_d_ = DeviceBuffer(D_ * sizeof(float), scale.data(), "scale");
  shift_d_ = DeviceBuffer(D_ * sizeof(float), shift.data(), "shift");
}

template <class Args>
void ServeRing::fill_dense_args(Args& a, const std::vector<DenseServeLayer>& layers, const ServeStats& stats) const {
  a.nslots = nslots_;
  a.D = D_;
  a.nl = (int)layers.size();
  for (size_t i = 0; i < layers.size(); ++i) a.L[i] = layers[i];
  a.idle_ticks = (uint64_t)(idle_s_ * 100e6);   // s_memrealtime runs at 100 MHz
  a.stats = stats.device();
  a.ctl = ctl_d_;
  a.req = req_d_;
  a.res = res_d_;
  a.scale = scale_d_.as<float>();
  a.shift = shift_d_.as<float>();
}

AEServe::AEServe(int device, int nslots, const std::vector<float>& weights, const int dims[3], const int acts[4],
                 const std::vector<float>& scale, const std::vector<float>& shift, float threshold,
                 double idle_seconds)
    : ServeRing(device, nslots, dims[0], idle_seconds, 32), threshold_(threshold) {   // no key word: all 32
  name_ = "AEServe";
  for (int i = 0; i < 3; ++i) dims_[i] = dims[i];
  for (int i = 0; i < 4; ++i) acts_[i] = acts[i];
  const int D = dims[0], n1 = dims[1], n2 = dims[2];
  if (D < 1 || D > 32 || n1 < 1 || n1 > 16 || n2 < 1 || n2 > 16)
    throw std::invalid_argument("AEServe: dims exceed the serving kernel (D <= 32, hidden <= 16)");
  const size_t nw = (size_t)D * n1 + n1 + (size_t)n1 * n2 + n2 + (size_t)n2 * n2 + n2 + (size_t)n2 * D + D;
  if (weights.size() != nw) throw std::invalid_argument("AEServe: weight vector has the wrong length");
  wts_d_ = DeviceBuffer(nw * sizeof(float), weights.data(), "weights");
  upload_affine(scale, shift, "AEServe");
  launch();
}

hipError_t AEServe::launch_kernel() {
  return ae_serve_launch(ctl_d_, req_d_, res_d_, nslots_, wts_d_.as<float>(), scale_d_.as<float>(),
                         shift_d_.as<float>(), dims_, acts_, threshold_, idle_s_, stream_);
}

int DenseServe::checked_D(const std::vector<float>& image, const std::vector<DenseServeLayer>& layers, int D,
                          const std::vector<float>& scale, const std::vector<float>& shift) {
  if (layers.empty() || layers.size() > (size_t)DSV_MAXLAYERS)
    throw std::invalid_argument("DenseServe: the stack must have 1..8 Dense layers");
  const char* why = dense_serve_check(layers.data(), (int)layers.size(), D, (int64_t)image.size());
  if (why[0]) throw std::invalid_argument(std::string("DenseServe: ") + why);
  check_affine(scale, shift, D, "DenseServe");
  return D;
}

DenseServe::DenseServe(int device, int nslots, const std::vector<float>& image,
                       const std::vector<DenseServeLayer>& layers, int D, const std::vector<float>& scale,
                       const std::vector<float>& shift, float threshold, double idle_seconds)
    : ServeRing(device, nslots, checked_D(image, layers, D, scale, shift), idle_seconds, 32) {   // no key word: all 32
  name_ = "DenseServe";
  DenseServeArgs& a = args_;
  upload_affine(scale, shift, name_);
  fill_dense_args(a, layers, stats_);
  a.img_floats = (int)image.size();
  a.threshold = threshold;
  in_lds_ = dense_serve_in_lds(a.L, a.nl);
  img_d_ = DeviceBuffer(image.size() * sizeof(float), image.data(), "weight image");
  a.img = img_d_.as<float>();
  launch();
}

hipError_t DenseServe::launch_kernel() { return dense_serve_launch(args_, stream_); }

int DenseFleetServe::checked_D(const float* images, int64_t n_models, int64_t stride, int64_t img_floats,
                               const std::vector<DenseServeLayer>& layers, int D, const std::vector<float>& scale,
                               const std::vector<float>& shift, const std::vector<float>& thresholds) {
  if (layers.empty() || layers.size() > (size_t)DSV_MAXLAYERS)
    throw std::invalid_argument("DenseFleetServe: the stack must have 1..8 Dense layers");
  const char* why = dense_fleet_serve_check(layers.data(), (int)layers.size(), D, img_floats, stride, n_models);
  if (why[0]) throw std::invalid_argument(std::string("DenseFleetServe: ") + why);
  if (!images) throw std::invalid_argument("DenseFleetServe: no images");
  if ((int64_t)thresholds.size() != n_models) throw std::invalid_argument("DenseFleetServe: one threshold per model");
  check_affine(scale, shift, D, "DenseFleetServe");
  return D;
}

DenseFleetServe::DenseFleetServe(int device, int nslots, const float* images, int64_t n_models, int64_t stride,
                                 int64_t img_floats, const std::vector<DenseServeLayer>& layers, int D,
                                 const std::vector<float>& scale, const std::vector<float>& shift,
                                 const std::vector<float>& thresholds, double idle_seconds)
    // request word 31 carries the model index
    : ServeRing(device, nslots, checked_D(images, n_models, stride, img_floats, layers, D, scale, shift, thresholds),
                idle_seconds, DSV_FLEET_MAXD) {
  name_ = "DenseFleetServe";
  DenseFleetServeArgs& a = args_;
  upload_affine(scale, shift, name_);
  fill_dense_args(a, layers, stats_);
  a.img_floats = (int)img_floats;
  a.stride = (int)stride;
  a.n_models = (int)n_models;
  img_d_ = DeviceBuffer((size_t)n_models * (size_t)stride * sizeof(float), images, "weight images");
  thr_d_ = DeviceBuffer((size_t)n_models * sizeof(float), thresholds.data(), "thresholds");
  a.img = img_d_.as<float>();
  a.thr = thr_d_.as<float>();
  launch();
}

hipError_t DenseFleetServe::launch_kernel() { return dense_fleet_serve_launch(args_, stream_); }

int64_t DenseFleetServe::first_bad_index(const uint32_t* models, int64_t k) const {
  const uint32_t M = (uint32_t)args_.n_models;
  for (int64_t i = 0; i < k; ++i)
    if (models[i] >= M) return i;
  return -1;
}

void DenseFleetServe::infer(const float* rows, const uint32_t* models, int k, float* scores, uint32_t* flags,
                            float* recon, double timeout_s) {
  if (k > 0 && !models) throw std::invalid_argument("DenseFleetServe: one model index per row");
  // the kernel trusts word 31: nothing is published unless every index names a model
  const int64_t bad = first_bad_index(models, k);
  if (bad >= 0)
    throw std::invalid_argument("DenseFleetServe: model index " + std::to_string(models[bad]) + " of row " +
                                std::to_string(bad) + " is outside [0, " + std::to_string(args_.n_models) + ")");
  ServeRing::infer(rows, k, scores, flags, recon, timeout_s, models);
}

void DenseFleetServe::set_image(int64_t i, const float* image) {
  if (i < 0 || i >= (int64_t)args_.n_models)
    throw std::invalid_argument("DenseFleetServe: model index " + std::to_string(i) + " is outside [0, " +
                                std::to_string(args_.n_models) + ")");
  halt();
  ck(hipSetDevice(device_), "hipSetDevice");
  ck(hipMemcpy(img_d_.as<float>() + (size_t)i * (size_t)args_.stride, image, (size_t)args_.stride * sizeof(float),
               hipMemcpyHostToDevice),
     "copy weight image");
}

void DenseFleetServe::set_images(const float* images) {
  halt();
  ck(hipSetDevice(device_), "hipSetDevice");
  ck(hipMemcpy(img_d_.as<float>(), images, (size_t)args_.n_models * (size_t)args_.stride * sizeof(float),
               hipMemcpyHostToDevice),
     "copy weight images");
}

int LSTMServe::checked_lanes(int device, int lanes, const std::vector<LstmServeLayer>& layers, int D, int T) {
  if (lanes == 1) return lanes;
  if (lanes < 1 || lanes > LSW_MAXLANES)
    throw std::invalid_argument(std::string("LSTMServe: lanes must be 1..") + std::to_string((int)LSW_MAXLANES));
  if (!layers.empty() && layers.size() <= (size_t)LS_MAXLAYERS) {   // else refused below: 1..8 layers
    LstmServeArgs a{};
    a.nl = (int)layers.size();
    for (size_t i = 0; i < layers.size(); ++i) a.L[i] = layers[i];
    a.D = D;
    a.T = T;
    if (lstm_serve_select(a) != LSK_WIDE)
      throw std::invalid_argument("LSTMServe: only the streamed-weight (wide) kernel runs on several lanes");
  }
  // a lane occupies a whole CU for as long as the server lives; the card also hosts the
  // autoencoder scorer and training
  int cus = 0;
  ck(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device), "multiprocessor count");
  if (lanes > cus / 2)
    throw std::invalid_argument("LSTMServe: lanes must not exceed half the device's compute units (" +
                                std::to_string(cus / 2) + " here)");
  return lanes;
}

LSTMServe::LSTMServe(int device, int nslots, const std::vector<float>& weights,
                     const std::vector<LstmServeLayer>& layers, int D, int T, int nkeys,
                     const std::vector<float>& scale, const std::vector<float>& shift, float threshold,
                     double idle_seconds, int lanes)
    // request word 31 carries the car key
    : ServeRing(device, nslots, D, idle_seconds, 31, checked_lanes(device, lanes, layers, D, T)) {
  name_ = "LSTMServe";
  if (layers.empty() || layers.size() > (size_t)LS_MAXLAYERS) throw std::invalid_argument("LSTMServe: 1..8 layers");
  if (T < 1 || T > 64) throw std::invalid_argument("LSTMServe: look_back must be 1..64");
  if (nkeys < 1) throw std::invalid_argument("LSTMServe: nkeys must be >= 1");
  for (const auto& L : layers) {   // every offset inside the weight vector
    const int64_t G = L.kind == LS_LSTM ? 4 * (int64_t)L.u : L.u;
    if (L.kind == LS_REPEAT) continue;
    if (L.woff < 0 || (int64_t)L.woff + (int64_t)L.in * G > (int64_t)weights.size() || L.boff < 0 ||
        (int64_t)L.boff + G > (int64_t)weights.size() ||
        (L.kind == LS_LSTM && (L.uoff < 0 || (int64_t)L.uoff + (int64_t)L.u * G > (int64_t)weights.size())))
      throw std::invalid_argument("LSTMServe: a layer's weights lie outside the weight vector");
  }
  check_affine(scale, shift, D, "LSTMServe");
  LstmServeArgs& a = args_;
  a.nslots = nslots_;
  a.lanes = lanes_;
  a.nw = (int)weights.size();
  a.nl = (int)layers.size();
  for (size_t i = 0; i < layers.size(); ++i) a.L[i] = layers[i];
  a.D = D;
  a.T = T;
  a.nkeys = nkeys;
  a.threshold = threshold;
  a.idle_ticks = (uint64_t)(idle_seconds * 100e6);   // s_memrealtime runs at 100 MHz
  // every limit of the kernel that will run, before anything is allocated on the device
  kernel_ = lstm_serve_select(a);
  if (kernel_ == LSK_WIDE) {
    const char* why = lstm_serve_wide_check(a);
    if (why[0]) throw std::invalid_argument(std::string("LSTMServe: ") + why);
    if (lstm_serve_wide_lds_bytes(a) + 16 * 1024 > 160 * 1024)
      throw std::invalid_argument("LSTMServe: the window's sequences do not fit the forecaster's LDS");
  } else if (lanes_ > 1) {   // repeated: SML_LSTM_SERVE_GENERIC may have changed between the two looks
    throw std::invalid_argument("LSTMServe: only the streamed-weight (wide) kernel runs on several lanes");
  } else if (lstm_serve_lds_bytes((int)weights.size()) > 160 * 1024) {
    throw std::invalid_argument("LSTMServe: the weights do not fit the scorer's LDS");
  }
  wts_d_ = DeviceBuffer(weights.size() * sizeof(float), weights.data(), "weights");
  upload_affine(scale, shift, name_);
  a.ctl = ctl_d_;
  a.req = req_d_;
  a.res = res_d_;
  a.wts = wts_d_.as<float>();
  a.scale = scale_d_.as<float>();
  a.shift = shift_d_.as<float>();
  if (kernel_ == LSK_WIDE) build_wide(weights);
  hist_d_ = DeviceBuffer((size_t)nkeys * T * D * sizeof(float), nullptr, "windows");
  hcount_d_ = DeviceBuffer((size_t)nkeys * sizeof(int), nullptr, "counts");
  lastpred_d_ = DeviceBuffer((size_t)nkeys * D * sizeof(float), nullptr, "forecasts");
  a.hist = hist_d_.as<float>();
  a.hcount = hcount_d_.as<int>();
  a.lastpred = lastpred_d_.as<float>();
  reset_keys();   // zeroes the key state and launches the resident kernel
}

void LSTMServe::build_wide(const std::vector<float>& weights) {
  // one host image, one allocation, one copy on the server's stream: per LSTM layer the bf16
  // image of W [Kp, 4 up], of U [up, 4 up], then the fp32 bias [4 up] (all 16-byte aligned:
  // 4 up is a multiple of 128)
  LstmServeArgs& a = args_;
  size_t off[LS_MAXLAYERS][3], total = 0;
  int li = 0;
  for (int l = 0; l < a.nl; ++l) {
    const LstmServeLayer& L = a.L[l];
    if (L.kind != LS_LSTM) continue;
    const size_t up = lstm_serve_wide_pad(L.u), kp = lstm_serve_wide_pad(L.in), G = 4 * up;
    off[li][0] = total;
    total += kp * G * sizeof(uint16_t);
    off[li][1] = total;
    total += up * G * sizeof(uint16_t);
    off[li][2] = total;
    total += G * sizeof(float);
    ++li;
  }
  std::vector<unsigned char> img(total, 0);
  li = 0;
  for (int l = 0; l < a.nl; ++l) {
    const LstmServeLayer& L = a.L[l];
    if (L.kind != LS_LSTM) continue;
    const int up = lstm_serve_wide_pad(L.u), kp = lstm_serve_wide_pad(L.in);
    lstm_serve_wide_image(weights.data() + L.woff, L.in, L.u, kp, up,
                          reinterpret_cast<uint16_t*>(img.data() + off[li][0]));
    lstm_serve_wide_image(weights.data() + L.uoff, L.u, L.u, up, up,
                          reinterpret_cast<uint16_t*>(img.data() + off[li][1]));
    float* b = reinterpret_cast<float*>(img.data() + off[li][2]);
    for (int q = 0; q < 4; ++q)
      for (int j = 0; j < L.u; ++j) b[q * up + j] = weights[(size_t)L.boff + q * L.u + j];
    ++li;
  }
  wide_d_ = DeviceBuffer(total, nullptr, "weight images");
  unsigned char* const wide = wide_d_.as<unsigned char>();
  ck(hipMemcpyAsync(wide, img.data(), total, hipMemcpyHostToDevice, stream_), "copy weight images");
  ck(hipStreamSynchronize(stream_), "sync");
  for (int i = 0; i < li; ++i) {
    a.wide_w[i] = reinterpret_cast<const uint16_t*>(wide + off[i][0]);
    a.wide_u[i] = reinterpret_cast<const uint16_t*>(wide + off[i][1]);
    a.wide_b[i] = reinterpret_cast<const float*>(wide + off[i][2]);
  }
  const LstmServeWideDims d = lstm_serve_wide_dims(a);
  wide_zx_d_ = DeviceBuffer((size_t)lanes_ * d.rows * d.gmax * sizeof(float), nullptr,   // one scratch per lane
                            "projection scratch");
  a.wide_zx = wide_zx_d_.as<float>();
}

const char* LSTMServe::kernel() const {
  static const char* const names[] = {"ref1", "pipe", "generic", "wide"};
  return names[kernel_];
}

void LSTMServe::reset_keys() {
  // the resident kernel reads and writes the key state: stop it first (flag + drain the
  // stream), so the memsets never queue behind a kernel that only leaves at its idle timeout
  stop();
  mark_lane_events();
  ck(hipMemsetAsync(args_.hcount, 0, (size_t)args_.nkeys * sizeof(int), stream_), "memset counts");
  ck(hipMemsetAsync(args_.lastpred, 0, (size_t)args_.nkeys * args_.D * sizeof(float), stream_), "memset forecasts");
  ck(hipStreamSynchronize(stream_), "sync");
  launch();
}

hipError_t LSTMServe::launch_kernel() { return lstm_serve_launch(args_, stream_); }

uint64_t ServeRing::submit(const float* rows, int k, const uint32_t* keys, int lane) {
  uint64_t& head = head_[(size_t)lane];
  if (k <= 0) return head;
  if (k > nslots_) throw std::invalid_argument("serve: more rows than slots");
  // back-pressure: never overwrite a slot whose event is not done
  if (head + (uint64_t)k > (uint64_t)nslots_) wait_done(head + (uint64_t)k - (uint64_t)nslots_, 10.0, lane);
  const uint64_t first = head;
  for (int i = 0; i < k; ++i) {
    const uint64_t ev = first + (uint64_t)i;
    ServeReq& dst = slot_req(ev, lane);
    const uint64_t tag = (uint64_t)(uint32_t)(ev + 1) << 32;
    const float* row = rows + (size_t)i * D_;
    for (int j = 0; j < D_; ++j) {   // 8-byte atomic stores: a word is never seen half-written
      uint32_t bits;
      std::memcpy(&bits, &row[j], 4);
      __atomic_store_n(&dst.w[j], tag | bits, __ATOMIC_RELAXED);
    }
    if (keys) __atomic_store_n(&dst.w[31], tag | keys[i], __ATOMIC_RELAXED);
  }
  head += k;
  store_rel(&ctl_[lane].head, head);   // after the rows: the backlog path trusts rows below head
  return first;
}

bool ServeRing::complete(uint64_t seq, int lane) const {
  const ServeResult& r = slot_res(seq, lane);
  const uint32_t tag = (uint32_t)(seq + 1);
  for (int i = kServeScore; i < kServeWords; ++i)
    if ((uint32_t)(__atomic_load_n(&r.w[i], __ATOMIC_RELAXED) >> 32) != tag) return false;
  for (int i = 0; i < D_; ++i)
    if ((uint32_t)(__atomic_load_n(&r.w[i], __ATOMIC_RELAXED) >> 32) != tag) return false;
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  return true;
}

uint32_t ServeRing::word(uint64_t seq, int i, int lane) const {
  return (uint32_t)__atomic_load_n(&slot_res(seq, lane).w[i], __ATOMIC_RELAXED);
}

float ServeRing::score(uint64_t seq, int lane) const {
  const uint32_t b = word(seq, kServeScore, lane);
  float f;
  std::memcpy(&f, &b, 4);
  return f;
}

void ServeRing::mark_lane_events() {
  for (int l = 0; l < lanes_; ++l) done0_[(size_t)l] = load_acq(&ctl_[l].done);
}

std::vector<int64_t> ServeRing::lane_events() const {
  // the device stores `done` after the tagged result words that wait() polls, so a call can
  // return a moment before the last `done` lands: events the host has already gathered count too
  std::vector<int64_t> n((size_t)lanes_);
  for (int l = 0; l < lanes_; ++l) {
    const uint64_t done = std::max(load_acq(&ctl_[l].done), complete_[(size_t)l]);
    n[(size_t)l] = (int64_t)(done - done0_[(size_t)l]);
  }
  return n;
}

void ServeRing::wait_done(uint64_t n, double timeout_s, int lane) {
  const auto t0 = std::chrono::steady_clock::now();
  uint32_t spins = 0;
  const uint64_t* done = &ctl_[lane].done;
  while (load_acq(done) < n) {
    cpu_relax();
    if ((++spins & 0x3ff) == 0) {
      if (hipStreamQuery(stream_) == hipSuccess && load_acq(done) < n) launch();
      const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      if (el > timeout_s) throw std::runtime_error(std::string(name_) + ": timed out waiting for free slots");
    }
  }
}

void ServeRing::wait(uint64_t seq_end, double timeout_s, int lane) {
  const auto t0 = std::chrono::steady_clock::now();
  uint32_t spins = 0;
  uint64_t& done = complete_[(size_t)lane];
  uint64_t ev = done < seq_end ? std::max<uint64_t>(done, seq_end > (uint64_t)nslots_ ?
                                                              seq_end - (uint64_t)nslots_ : 0)
                               : seq_end;
  while (ev < seq_end) {
    if (complete(ev, lane)) {
      ++ev;
      continue;
    }
    cpu_relax();
    if ((++spins & 0x3ff) == 0) {
      // the kernel exits after idle_seconds without work, or may have raced its
      // exit with our publish: relaunch it once it has really finished (every lane
      // resumes at its `done`, written after each event's result stores were issued)
      if (hipStreamQuery(stream_) == hipSuccess && !complete(ev, lane)) launch();
      const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      if (el > timeout_s) throw std::runtime_error(std::string(name_) + ": timed out waiting for results");
    }
  }
  done = std::max(done, seq_end);
}

void ServeRing::copy_result(uint64_t seq, int lane, int row, float* scores, uint32_t* flags, float* recon) const {
  if (scores) scores[row] = score(seq, lane);
  if (flags) flags[row] = word(seq, kServeFlag, lane);
  if (recon)
    for (int j = 0; j < D_; ++j) {
      const uint32_t b = word(seq, j, lane);
      std::memcpy(&recon[(size_t)row * D_ + j], &b, 4);
    }
}

void ServeRing::infer(const float* rows, int k, float* scores, uint32_t* flags, float* recon, double timeout_s,
                      const uint32_t* keys) {
  if (lanes_ > 1) {
    if (!keys) throw std::invalid_argument("serve: a ring with several lanes needs one key per row");
    infer_lanes(rows, k, scores, flags, recon, timeout_s, keys);
    return;
  }
  int off = 0;
  while (off < k) {
    const int n = std::min(k - off, nslots_);
    const uint64_t first = submit(rows + (size_t)off * D_, n, keys ? keys + off : nullptr);
    wait(first + n, timeout_s);
    for (int i = 0; i < n; ++i) copy_result(first + (uint64_t)i, 0, off + i, scores, flags, recon);
    off += n;
  }
}

void ServeRing::infer_lanes(const float* rows, int k, float* scores, uint32_t* flags, float* recon,
                            double timeout_s, const uint32_t* keys) {
  // lane l's j-th event of this batch: sequence number base[l] + j, batch row order[start[l] + j].
  // Every earlier call gathered all it published, so base[l] is also the lane's oldest
  // event whose result slot is still needed.
  const ServeLanePartition part = serve_lane_partition(keys, k, lanes_);
  const std::vector<uint64_t> base(head_);
  std::vector<int> pub((size_t)lanes_, 0), got((size_t)lanes_, 0);
  // the lane's oldest ungathered event: wait for it (block), or take it only if it has landed
  auto gather = [&](int l, bool block) {
    const uint64_t ev = base[(size_t)l] + (uint64_t)got[(size_t)l];
    if (block)
      wait(ev + 1, timeout_s, l);
    else if (!complete(ev, l))
      return false;
    copy_result(ev, l, part.order[(size_t)(part.start[(size_t)l] + got[(size_t)l])], scores, flags, recon);
    ++got[(size_t)l];
    // the lane's complete prefix moves with every gathered event, on either path: once ev is
    // gathered its slot may be published again (event ev + nslots), and a later wait() that
    // started below ev + 1 would look for ev's tag in a slot that no longer carries it
    complete_[(size_t)l] = std::max(complete_[(size_t)l], ev + 1);
    return true;
  };
  for (int i = 0; i < k; ++i) {   // one walk in batch order: a lane sees its keys' events in order
    const int l = serve_lane_of(keys[i], lanes_);
    if (pub[(size_t)l] - got[(size_t)l] == nslots_) {
      // this lane's ring is full (its result slots too): block on its oldest event, the one
      // the device reaches first, then take whatever else has landed.  The other lanes
      // already hold their share of the rows walked so far and keep draining meanwhile.
      gather(l, true);
      while (got[(size_t)l] < pub[(size_t)l] && gather(l, false)) {
      }
    }
    submit(rows + (size_t)i * D_, 1, keys + i, l);
    ++pub[(size_t)l];
  }
  for (int l = 0; l < lanes_; ++l)
    while (got[(size_t)l] < pub[(size_t)l]) gather(l, true);
}

std::vector<int64_t> ServeRing::latency_run(const float* rows, int n, int64_t gap_ns, std::vector<int64_t>* dev_ns,
                                            const uint32_t* keys) {
  if (lanes_ > 1 && !keys) throw std::invalid_argument("serve: a ring with several lanes needs one key per row");
  std::vector<int64_t> lat(n);
  if (dev_ns) dev_ns->assign(n, 0);
  auto next = std::chrono::steady_clock::now();
  for (int i = 0; i < n; ++i) {
    while (std::chrono::steady_clock::now() < next) cpu_relax();
    const int l = lanes_ > 1 ? serve_lane_of(keys[i], lanes_) : 0;   // the lane that runs the event
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t s = submit(rows + (size_t)i * D_, 1, keys ? keys + i : nullptr, l);
    wait(s + 1, 10.0, l);
    const auto t1 = std::chrono::steady_clock::now();
    lat[i] = std::chrono::duration_cast<std::chrono::nanoseconds>(t1 - t0).count();
    if (dev_ns) {
      // 100 MHz ticks -> ns, packed: [total | load | compute] in three 21-bit fields (ns / 10)
      const int64_t tot = word(s, kServeTDone, l), ld = word(s, kServeTLoad, l),
                    cp = (int64_t)word(s, kServeTComp, l) - (int64_t)word(s, kServeTLoad, l);
      (*dev_ns)[i] = (std::min<int64_t>(tot, 0x1fffff) << 42) | (std::min<int64_t>(ld, 0x1fffff) << 21) |
                     std::min<int64_t>(cp, 0x1fffff);
    }
    next = t0 + std::chrono::nanoseconds(gap_ns);
  }
  return lat;
}

std::vector<uint64_t> ServeRing::debug_state(uint64_t seq, int lane) const {
  if (lane < 0 || lane >= lanes_) throw std::out_of_range("serve: lane outside [0, lanes)");
  const ServeCtl& c = ctl_[lane];
  std::vector<uint64_t> v = {__atomic_load_n(&c.head, __ATOMIC_ACQUIRE), __atomic_load_n(&c.done, __ATOMIC_ACQUIRE),
                             __atomic_load_n(&ctl_->stop, __ATOMIC_ACQUIRE), __atomic_load_n(&c.alive, __ATOMIC_ACQUIRE),
                             launches_, hipStreamQuery(stream_) == hipSuccess ? 1u : 0u};
  const ServeResult& r = slot_res(seq, lane);
  for (size_t i = 0; i < sizeof(ServeResult) / 8; ++i) v.push_back(__atomic_load_n(&r.w[i], __ATOMIC_ACQUIRE));
  const ServeReq& q = slot_req(seq, lane);
  for (int i = 0; i < 32; ++i) v.push_back(__atomic_load_n(&q.w[i], __ATOMIC_ACQUIRE));
  return v;
}

void ServeRing::stop() {
  if (!ctl_) return;
  __atomic_store_n(&ctl_->stop, 1u, __ATOMIC_RELEASE);
  if (stream_) (void)hipStreamSynchronize(stream_);
}

}  // namespace sml
