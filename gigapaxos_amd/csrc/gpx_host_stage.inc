// Staging of the control-plane host-pointer calls: the temporary device columns of one call, the copies in and out, and
// the call's status.  Needs: gpx_engine (sB, arena_*), xfer, g_err, HIPQ.

namespace {

/* One synchronous host-pointer call.  Its device columns come out of one engine-owned arena that is rewound at the start
 * of every call - a hipMalloc / hipFree pair per buffer cost more than the kernels of a small call.  The arena grows
 * between calls to the largest demand seen; a call that outgrows it takes its extra buffers from hipMalloc for that call
 * only, and so does every buffer of a nested call and of a call that stays outside the arena (arena = false: the
 * lifecycle calls, whose 2^18-record chunks would pin tens of megabytes in it).
 *
 * The first failed allocation (GPX_ENOMEM) or runtime call (GPX_EDEVICE) is kept in `rc` and turns every later request
 * into a no-op that returns null: a caller asks ready() once before it launches and returns what sync() / fetch() give.
 * ready() is also where the input columns are copied: every fill of the call is queued before the first copy, as the
 * calls always did - a copy from pageable memory waits for the stream, so a copy between two fills costs the host the
 * latency of a fill each time (8 - 35 us per call where it was tried, profiles/r14_host_ctl_stage.txt).
 * Whatever way the call leaves, the destructor waits for anything still queued before the arena goes to the next call,
 * and frees the per-call buffers. */
struct CtlStage {
  static constexpr size_t ALL = ~(size_t)0;
  gpx_engine* h;
  int rc = GPX_OK;
  bool owner, queued = false;
  std::vector<void*> extra;
  struct Out {
    void* host;
    const void* dev;
    size_t count, elt;
    bool optional;
  };
  std::vector<Out> outs;
  struct In {
    void* dev;
    const void* host;
    size_t bytes;
  };
  std::vector<In> ins; /* input columns not copied yet */

  explicit CtlStage(gpx_engine* h_, bool arena = true) : h(h_), owner(arena && !h_->arena_busy) {
    if (!owner) return;
    h->arena_busy = true;
    if (h->arena_want > h->arena_cap) {
      /* nothing is in flight on the old block: no call leaves with work queued */
      if (h->arena) HIPQ(hipFree(h->arena));
      h->arena = nullptr;
      h->arena_cap = 0;
      const size_t want = h->arena_want + h->arena_want / 4;
      void* q = nullptr;
      if (hipMalloc(&q, want) == hipSuccess) {
        h->arena = (char*)q;
        h->arena_cap = want;
      }
    }
    h->arena_used = 0;
    h->arena_demand = 0;
  }
  ~CtlStage() {
    if (queued) HIPQ(hipStreamSynchronize(h->sB));
    for (void* q : extra) HIPQ(hipFree(q));
    if (owner) {
      h->arena_want = std::max(h->arena_want, h->arena_demand);
      h->arena_busy = false;
    }
  }
  CtlStage(const CtlStage&) = delete;
  CtlStage& operator=(const CtlStage&) = delete;

  bool fail(int code, const char* what, hipError_t err) {
    if (rc == GPX_OK) {
      rc = code;
      snprintf(g_err, sizeof(g_err), "%s -> %s", what, hipGetErrorString(err));
    }
    return false;
  }
  bool did(hipError_t err, const char* what) {
    queued = true;
    return err == hipSuccess || fail(GPX_EDEVICE, what, err);
  }

  /* a device column of `count` elements.  Zero-filled: deterministic contents where a kernel leaves a slot unwritten
   * (records of frames refused with GPX_W_CAPACITY).  The fill is on the engine's stream: the engine streams are
   * non-blocking, a null-stream memset would not be ordered before the copies / kernels that follow. */
  void* tmp_bytes(size_t count, size_t elt, bool zero) {
    if (rc != GPX_OK) return nullptr;
    const size_t bytes = (std::max<size_t>(count, 1) * elt + 255) & ~(size_t)255;
    void* q = nullptr;
    if (owner) h->arena_demand += bytes;
    if (owner && h->arena && h->arena_used + bytes <= h->arena_cap) {
      q = h->arena + h->arena_used;
      h->arena_used += bytes;
    } else {
      const hipError_t err = hipMalloc(&q, bytes);
      if (err != hipSuccess) return fail(GPX_ENOMEM, "hipMalloc", err), nullptr;
      extra.push_back(q);
    }
    if (zero) {
      queued = true;
      const hipError_t err = hipMemsetAsync(q, 0, bytes, h->sB);
      if (err != hipSuccess) return fail(GPX_ENOMEM, "hipMemsetAsync", err), nullptr;
    }
    return q;
  }
  template <typename T>
  T* tmp(size_t count, bool zero = true) { return (T*)tmp_bytes(count, sizeof(T), zero); }

  /* plain copies on the engine's stream, for what is no whole column */
  void h2d(void* dev, const void* host, size_t bytes) {
    if (rc == GPX_OK) did(xfer(h, dev, host, bytes, hipMemcpyHostToDevice, h->sB), "copy to the device");
  }
  void d2h(void* host, const void* dev, size_t bytes) {
    if (rc == GPX_OK) did(xfer(h, host, dev, bytes, hipMemcpyDeviceToHost, h->sB), "copy from the device");
  }

  /* clears engine-owned device memory on the engine's stream */
  void zero(void* dev, size_t bytes) {
    if (rc == GPX_OK) did(hipMemsetAsync(dev, 0, bytes, h->sB), "hipMemsetAsync");
  }

  /* this host column of `count` elements on the device (copied by ready()); in_opt: a null column stays null */
  template <typename T>
  T* in(const T* host, size_t count) {
    T* d = tmp<T>(count);
    if (d && count) ins.push_back(In{d, host, count * sizeof(T)});
    return d;
  }
  template <typename T>
  T* in_opt(const T* host, size_t count) { return host ? in(host, count) : nullptr; }

  /* a device column of `count` elements that goes back to `host`; out_opt: the kernel writes the column either way, a
   * null `host` only keeps it from being fetched */
  void* out_bytes(void* host, size_t count, size_t elt, bool optional = false) {
    void* d = tmp_bytes(count, elt, true);
    if (d) outs.push_back(Out{host, d, count, elt, optional});
    return d;
  }
  template <typename T>
  T* out(T* host, size_t count) { return (T*)out_bytes(host, count, sizeof(T)); }
  template <typename T>
  T* out_opt(T* host, size_t count) { return (T*)out_bytes(host, count, sizeof(T), true); }

  /* queues the first min(k, count) elements of the output column `dev` to its host pointer */
  void queue(const void* dev, size_t k = ALL) {
    for (const Out& o : outs)
      if (o.dev == dev) {
        const size_t m = std::min(k, o.count);
        if (m && !(o.optional && !o.host)) d2h(o.host, o.dev, m * o.elt);
        return;
      }
  }
  /* every column is there and filled: copies the inputs in; the status, to be tested before the launch */
  int ready() {
    for (const In& c : ins) h2d(c.dev, c.host, c.bytes);
    ins.clear();
    return rc;
  }
  /* waits for everything queued so far */
  int sync() {
    if (rc == GPX_OK && did(hipStreamSynchronize(h->sB), "hipStreamSynchronize")) queued = false;
    return rc;
  }
  /* the first k elements of each named output, one wait */
  int fetch(std::initializer_list<const void*> devs, size_t k = ALL) {
    for (const void* d : devs) queue(d, k);
    return sync();
  }
  /* what a _dev twin or a helper that queues work returned */
  int ran(int rc_dev) {
    queued = true;
    if (rc == GPX_OK) rc = rc_dev;
    return rc;
  }
};

}  // namespace
