// Part of api.hip (inside its anonymous namespace): THE allocation gate.  Every device buffer, every page-locked host buffer and every
// buffer of the host backend that a context, its keys or its matrices hold is asked for through gate_alloc and given back through
// gate_free -- no other hipMalloc / hipHostMalloc / cpu::h_alloc call exists in csrc/.  Per context the gate keeps the bytes held
// through it and their peak, the page-locked bytes (counted apart), a request counter, the byte limit (amsm_ctx_set_memory_limit)
// and the test countdown (amsm_ctx_fail_alloc_after).  It refuses BEFORE it calls the driver when the limit would be exceeded or
// the countdown fires; a refusal looks to the caller exactly like a failed driver call (null pointer, AMSM_E_OOM), so that every
// site takes the path it always took: AMSM_E_OOM where the buffer is required, the site's fallback where it is tolerated.
enum GateKind { GATE_DEVICE = 0, GATE_PINNED = 1, GATE_HOST = 2 };

struct GateEntry {
  amsm_ctx* ctx;  // null: the owning context is gone (or the buffer never had one) -- freed, credited to nobody
  size_t bytes;
  int kind;
};
// One lock for the gate's books (allocations are rare next to kernel launches).  The map holds every buffer that went through the
// gate: amsm_bases_free / amsm_matrix_free take no context, the owner is found here.
inline std::mutex& gate_mu() {
  static std::mutex m;
  return m;
}
inline std::unordered_map<void*, GateEntry>& gate_map() {
  static std::unordered_map<void*, GateEntry> m;
  return m;
}

void pool_release_all(amsm_ctx* c);  // below: the vector pool's free lists back to the driver

// Drain the context's streams: a REQUIRED allocation was refused, the call is about to return AMSM_E_OOM and launches nothing more
// -- whatever it (or an earlier MSM of the same batch) queued has run when the status reaches the caller (include/amsm.h: "the
// contract after AMSM_E_OOM").  Errors are not looked at here: the failing call reports AMSM_E_OOM, the next one finds what is sticky.
inline void gate_drain(amsm_ctx* c) {
  if (c->host_only) return;
  for (hipStream_t s : {c->s_prep, c->stream, c->s_tail, c->s_copy, c->s_tv})
    if (s) (void)hipStreamSynchronize(s);
}

// bytes of `kind` for context `c` (null: nobody's books, no limit, no hook).  tolerated: the caller has a fallback and says nothing.
// AMSM_OK and *out, or AMSM_E_OOM and *out == nullptr.
enum GateWhy { GATE_GRANTED = 0, GATE_BY_LIMIT = 1, GATE_BY_HOOK = 2, GATE_BY_DRIVER = 3 };
int gate_alloc(amsm_ctx* c, int kind, size_t bytes, bool tolerated, void** out, int* why = nullptr) {
  *out = nullptr;
  bool refuse = false;
  if (why) *why = GATE_GRANTED;
  if (c) {
    std::unique_lock<std::mutex> lk(gate_mu());
    MemGate& g = c->gate;
    g.requests++;
    if (g.fail_after == 0) {  // the test hook: this request, once
      g.fail_after = -1;
      g.refused_hook++;
      refuse = true;
      if (why) *why = GATE_BY_HOOK;
    } else {
      if (g.fail_after > 0) g.fail_after--;
      if (kind != GATE_PINNED && g.limit && g.held + bytes > g.limit) {
        // give the free lists back once (what amsm_dev_alloc does after a driver failure), then decide.  (The pool has its own lock,
        // taken without this one: pool_release_all credits the books through gate_free.)
        lk.unlock();
        if (!c->host_only) (void)hipStreamSynchronize(c->stream);
        pool_release_all(c);
        lk.lock();
        if (g.held + bytes > g.limit) {
          g.refused_limit++;
          refuse = true;
          if (why) *why = GATE_BY_LIMIT;
        }
      }
    }
    // the bytes are RESERVED in the same critical section that checked them (a key made on another thread must not pass the same
    // check meanwhile) and given back below if the driver fails
    if (!refuse) {
      if (kind == GATE_PINNED) {
        g.pinned += bytes;
      } else {
        g.held += bytes;
        g.peak = std::max(g.peak, g.held);
      }
    }
  }
  void* p = nullptr;
  if (!refuse) {
    if (kind == GATE_HOST) {
      if (posix_memalign(&p, 64, std::max<size_t>(bytes, 64)) != 0) p = nullptr;
    } else {
      const hipError_t e = kind == GATE_PINNED ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes);
      if (e != hipSuccess) {
        (void)hipGetLastError();  // the sticky error must not surface at an unrelated call's hipGetLastError
        p = nullptr;
      }
    }
    if (!p && why) *why = GATE_BY_DRIVER;
    if (!p && c) {
      std::lock_guard<std::mutex> lk(gate_mu());
      MemGate& g = c->gate;
      g.failed_driver++;
      if (kind == GATE_PINNED) g.pinned -= bytes;  // the reservation (the peak keeps it: it was never above the limit)
      else g.held -= bytes;
    }
  }
  if (!p) {
    if (c && !tolerated) gate_drain(c);
    return AMSM_E_OOM;
  }
  std::lock_guard<std::mutex> lk(gate_mu());
  gate_map()[p] = GateEntry{c, bytes, kind};
  *out = p;
  return AMSM_OK;
}

// Give back a buffer of gate_alloc (null: nothing); its owner, if it still lives, is credited.  The driver's status for device memory.
hipError_t gate_free(void* p) {
  if (!p) return hipSuccess;
  int kind = GATE_DEVICE;
  {
    std::lock_guard<std::mutex> lk(gate_mu());
    auto it = gate_map().find(p);
    if (it != gate_map().end()) {
      kind = it->second.kind;
      if (amsm_ctx* c = it->second.ctx) {
        if (kind == GATE_PINNED) c->gate.pinned -= it->second.bytes;
        else c->gate.held -= it->second.bytes;
      }
      gate_map().erase(it);
    }
  }
  if (kind == GATE_HOST) {
    free(p);
    return hipSuccess;
  }
  return kind == GATE_PINNED ? hipHostFree(p) : hipFree(p);
}

// The context a buffer is booked on (null: none, or gone): a key's later tables (its C-ABI copy) go on the books of the context that
// holds its table
amsm_ctx* gate_owner_of(const void* p) {
  std::lock_guard<std::mutex> lk(gate_mu());
  auto it = gate_map().find(const_cast<void*>(p));
  return it == gate_map().end() ? nullptr : it->second.ctx;
}

// The context goes away: what it still has on its books (keys, matrices, vectors the caller holds) stays allocated and is forgotten
void gate_forget_ctx(amsm_ctx* c) {
  std::lock_guard<std::mutex> lk(gate_mu());
  for (auto& kv : gate_map())
    if (kv.second.ctx == c) kv.second.ctx = nullptr;
}

// ---- the vector pool's books (amsm_dev_alloc / amsm_dev_free, api_entry_vec.inc) ----
inline size_t pool_round(size_t bytes) {  // 256-byte granules up to 1 MiB, 64-KiB granules above
  bytes = std::max<size_t>(bytes, 16);
  const size_t g = bytes <= ((size_t)1 << 20) ? 256 : 65536;
  return (bytes + g - 1) / g * g;
}
// Which context's bookkeeping a buffer belongs to.  Two contexts can share a GPU (a multi-device context that lists a device
// twice, two callers) and a wrapper may free a vector through the other one: the owner's `pool_size` entry and live-byte
// count must follow, and the buffer must not enter a free list whose stream-order argument (api_types.h) does not cover
// the consumer.  Every allocator operation takes this one lock (they are rare next to kernel launches).
std::mutex g_pool_mu;
inline std::unordered_map<void*, amsm_ctx*>& pool_owner() {
  static std::unordered_map<void*, amsm_ctx*> m;
  return m;
}
void pool_release_all(amsm_ctx* c) {
  std::lock_guard<std::mutex> lk(g_pool_mu);
  for (auto& kv : c->pool)
    for (void* p : kv.second) {
      (void)gate_free(p);
      c->pool_size.erase(p);
      pool_owner().erase(p);
    }
  c->pool.clear();
  c->pool_free_bytes = 0;
}
// the context goes away: buffers it handed out and never got back stay allocated (the caller still holds them) but no
// longer point at it
void pool_forget_ctx(amsm_ctx* c) {
  std::lock_guard<std::mutex> lk(g_pool_mu);
  for (auto& kv : c->pool_size) pool_owner().erase(kv.first);
  c->pool_size.clear();
  c->pool_live_bytes = 0;
}
