// fullprover.cpp -- FullProver / ProverResponse (include/k16_fullprover.hpp) on top of the k16 C ABI.
// Host-only C++; mirrors the control flow of rust-rapidsnark/rapidsnark/src/fullprover.cpp:80-260.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/k16.h"
#include <time.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include "../../include/k16_fullprover.hpp"

namespace {

bool log_on()
{
    const char* e = getenv("K16_LOG");
    return e && *e && *e != '0';
}
void log_line(const char* level, const char* msg)
{
    if (!log_on()) return;
    // same fields as the reference's log() (fullprover.cpp:41-78): UTC timestamp with milliseconds, level, message,
    // native_code, target -- as VALID JSON (the reference's line carries a stray quote after "native_code":"1")
    struct timespec ts;
    clock_gettime(CLOCK_REALTIME, &ts);
    struct tm tmv;
    gmtime_r(&ts.tv_sec, &tmv);
    char stamp[40];
    const size_t k = strftime(stamp, sizeof stamp, "%Y-%m-%dT%H:%M:%S", &tmv);
    snprintf(stamp + k, sizeof stamp - k, ".%03ldZ", ts.tv_nsec / 1000000L);
    printf("{\"timestamp\":\"%s\",\"level\":\"%s\",\"message\":\"%s\",\"native_code\":\"1\",\"target\":\"prover_service::k16\"}\n",
           stamp, level, msg);
    fflush(stdout);
}

// Devices behind one FullProver.  K16_DEVICES="0,1,2,3" puts one resident copy of the key on each listed GPU and lets
// prove() run on whichever is free; a device may be listed more than once ("0,0,0": three provers sharing one GPU, whose
// proofs overlap on it).  Default: the single device K16_DEVICE (0).  SURVEY 8(f).3: the pool lives behind the facade, so
// the Rust side only has to stop serialising prove() calls to use it.  K16_DEVICES=all: every GPU the process can see.
std::vector<int> device_list()
{
    std::vector<int> devs;
    if (const char* e = getenv("K16_DEVICES")) {
        if (strcmp(e, "all") == 0) { // one resident key per GPU of the node (BASELINE config 4: a proof per GPU per wave)
            const int n = k16_device_count();
            for (int d = 0; d < n; d++) devs.push_back(d);
            return devs; // empty without a device: the constructor then reports it
        }
        const char* p = e;
        while (*p) {
            char* end = nullptr;
            long  v   = strtol(p, &end, 10);
            if (end == p) break;
            devs.push_back((int)v);
            p = end;
            while (*p == ',' || *p == ' ') p++;
        }
    }
    if (devs.empty()) {
        const char* e = getenv("K16_DEVICE");
        devs.push_back(e ? atoi(e) : 0);
    }
    return devs;
}

// k16_fullprover_last_rejection: what the calling thread's last prove through a FullProver was rejected for by the R1CS check
// (copied out of the slot while the thread still holds it: the pool serves concurrent callers, a per-object "last" would race)
struct Rejection {
    int      status   = K16_CHECK_NONE;
    uint64_t n_failed = 0;
    uint32_t lowest[K16_R1CS_REPORT_MAX];
};
thread_local Rejection t_rejection;

} // namespace

class FullProverImpl
{
public:
    struct Slot {
        k16_ctx*    ctx    = nullptr;
        k16_prover* prover = nullptr;
        k16_vk*     vk     = nullptr; // k16_fullprover_set_verify: the slot's verification key, built from the zkey and attached to its prover
        k16_r1cs*   r1cs   = nullptr; // k16_fullprover_set_r1cs: the slot's copy of the circuit, attached to its prover
        int         device = 0;
        bool        busy   = false;
        bool        dead   = false; // a device fault hit this slot and rebuilding it failed: never handed out again
    };
    std::vector<Slot>       slots;
    std::string             zkey_path; // to rebuild a slot after a device fault
    // k16_fullprover_set_verify: every proof is checked on the GPU before it is handed out (include/k16.h, verified proving);
    // a rejected proof -- the witness does not satisfy the circuit -- is answered with INVALID_INPUT / K16_ERR_FORMAT
    bool                    verify = false;
    // k16_fullprover_set_r1cs: every witness is checked against the circuit under its proof (include/k16.h, checked proving); one
    // that breaks a constraint, or is refused, is answered with INVALID_INPUT / K16_ERR_FORMAT.  Empty: off
    std::string             r1cs_path;
    std::mutex              mu;
    std::condition_variable cv;

    ~FullProverImpl()
    {
        for (Slot& s : slots) drop(&s);
    }
    static void drop(Slot* s)
    {
        if (s->prover) k16_prover_destroy(s->prover);
        if (s->vk) k16_vk_destroy(s->vk);
        if (s->r1cs) k16_r1cs_destroy(s->r1cs);
        if (s->ctx) k16_ctx_destroy(s->ctx);
        s->prover = nullptr;
        s->vk     = nullptr;
        s->r1cs   = nullptr;
        s->ctx    = nullptr;
    }
    // verification on: the slot's key from the zkey's sections 2 and 3, attached to its prover
    int attach_vk(Slot* s) const
    {
        if (!verify || s->vk) return K16_OK;
        int rc = k16_vk_create_from_zkey_file(s->ctx, zkey_path.c_str(), &s->vk);
        if (rc == K16_OK) rc = k16_prover_set_vk(s->prover, s->vk);
        return rc;
    }
    static void detach_vk(Slot* s)
    {
        if (s->prover) (void)k16_prover_set_vk(s->prover, nullptr);
        if (s->vk) k16_vk_destroy(s->vk);
        s->vk = nullptr;
    }
    // checking on: the slot's own copy of the circuit, attached to its prover
    int attach_r1cs(Slot* s) const
    {
        if (r1cs_path.empty() || s->r1cs) return K16_OK;
        int rc = k16_r1cs_create(s->ctx, r1cs_path.c_str(), &s->r1cs);
        if (rc == K16_OK) rc = k16_prover_set_r1cs(s->prover, s->r1cs);
        return rc;
    }
    static void detach_r1cs(Slot* s)
    {
        if (s->prover) (void)k16_prover_set_r1cs(s->prover, nullptr);
        if (s->r1cs) k16_r1cs_destroy(s->r1cs);
        s->r1cs = nullptr;
    }
    // After a prove call on the slot, while the caller still holds it.  rc: the call's status, or REJECTED -- a proof was made
    // and the pairing check rejects it.  The R1CS check's finding goes into the calling thread's record; a rejection by either
    // check is answered with K16_ERR_FORMAT.  Nothing attached, a failed call: status NONE.
    static constexpr int REJECTED = -1000;
    int after_prove(Slot* s, int rc) const
    {
        const bool by_pairing = rc == REJECTED;
        const bool by_check   = rejected_by_check(s, by_pairing ? 0 : rc);
        return (by_pairing || (by_check && rc >= 0)) ? (int)K16_ERR_FORMAT : rc;
    }
    bool rejected_by_check(Slot* s, int rc) const
    {
        t_rejection.status   = K16_CHECK_NONE;
        t_rejection.n_failed = 0;
        if (rc < 0 || !s->r1cs) return false;
        int      status = K16_CHECK_NONE;
        uint64_t n      = 0;
        if (k16_prover_last_check(s->prover, &status, &n, t_rejection.lowest, K16_R1CS_REPORT_MAX) != K16_OK) return false;
        if (status != K16_CHECK_BROKEN && status != K16_CHECK_WITNESS_REFUSED) return false;
        t_rejection.status   = status;
        t_rejection.n_failed = n;
        if (log_on()) {
            std::string msg = status == K16_CHECK_BROKEN ? "witness rejected by the R1CS check: " + std::to_string(n) + " broken constraints, lowest ["
                                                         : std::string("witness refused by the R1CS check: a value >= r, or wire 0 != 1 [");
            for (uint64_t k = 0; k < n && k < K16_R1CS_REPORT_MAX; k++) msg += (k ? "," : "") + std::to_string(t_rejection.lowest[k]);
            log_line("ERROR", (msg + "]").c_str());
        }
        return true;
    }
    // blocks until a prover is free; proofs of concurrent callers run on different slots.  nullptr: every slot is dead.
    Slot* acquire()
    {
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
            bool any_alive = false;
            for (Slot& s : slots) {
                if (s.dead) continue;
                any_alive = true;
                if (!s.busy) {
                    s.busy = true;
                    return &s;
                }
            }
            if (!any_alive) return nullptr;
            cv.wait(lk);
        }
    }
    // A HIP error during a proof (device fault, failed allocation, lost context) leaves the slot's context in an unknown
    // state: it is torn down and rebuilt from the key file in a fresh context before anybody else gets it.  If that
    // fails too the slot is marked dead; the other slots of the pool keep serving.
    void quarantine(Slot* s)
    {
        bool ok = false;
        try { // k16_* never throw (their own firewall); this guards the few host statements around them all the same
            drop(s);
            // (from the key FILE, not from a sibling's resident copy: after a device fault nothing on that device is trusted)
            ok = k16_ctx_create(s->device, &s->ctx) == K16_OK && k16_prover_create(s->ctx, zkey_path.c_str(), &s->prover) == K16_OK &&
                 attach_vk(s) == K16_OK && attach_r1cs(s) == K16_OK;
            if (ok) {
                int sharing = 0;
                for (auto& o : slots) sharing += o.device == s->device;
                if (sharing > 1) (void)k16_ctx_set_option(s->ctx, K16_OPT_SHARED_GPU, 1);
                if (slots.size() > 1) (void)k16_ctx_set_option(s->ctx, K16_OPT_YIELDING_WAITS, 1);
            }
        } catch (...) {
            ok = false;
        }
        if (!ok) {
            fprintf(stderr, "k16 FullProver: device %d could not be re-initialised after a fault; slot retired\n", s->device);
            drop(s);
            std::lock_guard<std::mutex> lk(mu);
            s->dead = true;
        }
    }
    void release(Slot* s) noexcept
    {
        try {
            std::lock_guard<std::mutex> lk(mu);
            s->busy = false;
            if (!s->prover) s->dead = true; // a slot without a prover must never be handed out
        } catch (...) { // a failing mutex lock: still never leave the slot marked busy
            s->busy = false;
        }
        cv.notify_all(); // also wakes waiters when the last live slot died
    }
    // Scope guard of one acquired slot: whatever leaves FullProver::prove -- a return, an exception out of the few host
    // statements between acquire and release -- gives the slot back (and retires it if it lost its prover on the way).
    // Without it an exception left the slot busy for ever and, with the default one-slot pool, every later prove()
    // waiting in acquire().
    struct Lease {
        FullProverImpl* impl;
        Slot*           slot;
        Lease(FullProverImpl* i) : impl(i), slot(i->acquire()) {}
        ~Lease()
        {
            if (slot) impl->release(slot);
        }
        Lease(const Lease&)            = delete;
        Lease& operator=(const Lease&) = delete;
    };
};

char const* const ProverResponse::empty_string = "";

ProverResponse::ProverResponse(ProverError _error)
    : type(ProverResponseType::ERROR), raw_json(ProverResponse::empty_string), error(_error), metrics(ProverResponseMetrics())
{
}

ProverResponse::ProverResponse(const char* _raw_json, ProverResponseMetrics _metrics)
    : type(ProverResponseType::SUCCESS), raw_json(_raw_json), error(ProverError::NONE), metrics(_metrics)
{
}

ProverResponse::~ProverResponse()
{
    if (raw_json != empty_string) free(const_cast<char*>(raw_json));
}

FullProver::FullProver(const char* _zkeyFileName) : impl(nullptr), state(FullProverState::ZKEY_FILE_LOAD_ERROR)
{
    if (!_zkeyFileName) return;
    FullProverImpl* p = nullptr;
    // nothing may throw across the FFI (bindgen callers cannot catch): allocation failures inside the std containers
    // used here and below end as ZKEY_FILE_LOAD_ERROR
    try {
        p            = new FullProverImpl();
        p->zkey_path = _zkeyFileName;
        const std::vector<int> devs = device_list();
        if (devs.empty()) {
            fprintf(stderr, "k16 FullProver: K16_DEVICES=all but no HIP device is visible; the prover has no CPU fallback\n");
            delete p;
            return;
        }
        for (int dev : devs) {
            FullProverImpl::Slot s;
            s.device = dev;
            // the n-th prover of a device sits n placeholder streams behind the first (include/k16.h k16_ctx_create_ex: which streams
            // of provers that share a GPU take turns on a dispatch pipe; +4.6 % proofs/s for two).  K16_POOL_STREAM_OFFSET=0 disables.
            int same_dev = 0;
            for (auto& o : p->slots) same_dev += o.device == dev;
            const char* off_env = getenv("K16_POOL_STREAM_OFFSET");
            const int   offset  = (off_env ? atoi(off_env) : 1) * same_dev;
            if (k16_ctx_create_ex(dev, ((offset % 4) + 4) % 4, &s.ctx) != K16_OK) {
                fprintf(stderr, "k16 FullProver: no usable MI355X / HIP device %d; the prover has no CPU fallback\n", dev);
                delete p;
                return;
            }
            // a device listed before already holds the key: share its read-only part (one upload, one window-table build)
            const k16_prover* sibling = nullptr;
            for (auto& o : p->slots)
                if (o.device == dev && o.prover) sibling = o.prover;
            int rc = sibling ? k16_prover_create_shared(s.ctx, sibling, &s.prover) : k16_prover_create(s.ctx, _zkeyFileName, &s.prover);
            if (rc != K16_OK) {
                // fullprover.cpp:91-100 : invalid_argument -> UNSUPPORTED_ZKEY_CURVE, system_error -> ZKEY_FILE_LOAD_ERROR
                state = (rc == K16_ERR_CURVE || rc == K16_ERR_FORMAT) ? FullProverState::UNSUPPORTED_ZKEY_CURVE
                                                                      : FullProverState::ZKEY_FILE_LOAD_ERROR;
                if (rc == K16_ERR_HIP || rc == K16_ERR_NO_DEVICE) fprintf(stderr, "k16 FullProver: %s\n", k16_last_error(s.ctx));
                k16_ctx_destroy(s.ctx);
                delete p;
                return;
            }
            p->slots.push_back(s);
        }
        // entries that share a GPU prove there at the same time: throughput tuning (include/k16.h, K16_OPT_SHARED_GPU)
        for (auto& s : p->slots) {
            int sharing = 0;
            for (auto& o : p->slots) sharing += o.device == s.device;
            if (sharing > 1) (void)k16_ctx_set_option(s.ctx, K16_OPT_SHARED_GPU, 1);
            // a pool means several callers waiting for proofs at once: their waits sleep instead of spinning (include/k16.h)
            if (p->slots.size() > 1) (void)k16_ctx_set_option(s.ctx, K16_OPT_YIELDING_WAITS, 1);
        }
    } catch (...) {
        delete p;
        state = FullProverState::ZKEY_FILE_LOAD_ERROR;
        return;
    }
    impl  = p;
    state = FullProverState::OK;
}

FullProver::~FullProver()
{
    if (impl) delete impl;
}

// The pool with the witness ALREADY IN MEMORY (include/k16.h k16_fullprover_prove_mem): what a service that keeps several
// GPUs busy binds instead of prove(path), which maps and parses a 43 MB .wtns file inside every call.  Same slot lease,
// same quarantine of a slot after a device fault; the status is the C ABI's instead of a ProverResponse.
extern "C" int k16_fullprover_prove_mem(const void* fullprover, const void* wtns_values, uint64_t n_values, char* out_json,
                                        size_t cap, int* prover_time_ms)
{
    try {
        // the object's two (private) fields, in the order the header -- the reference's -- declares them; bindgen sees the same
        struct Fields {
            FullProverImpl* impl;
            FullProverState state;
        } f;
        static_assert(sizeof(Fields) == sizeof(FullProver), "FullProver layout");
        if (prover_time_ms) *prover_time_ms = 0;
        if (!fullprover || !wtns_values || !out_json) return K16_ERR_ARG;
        memcpy(&f, fullprover, sizeof f);
        const Fields* fp = &f;
        if (fp->state != FullProverState::OK || !fp->impl) return K16_ERR_NO_DEVICE; // = PROVER_NOT_READY
        int        rc;
        const auto t0 = std::chrono::steady_clock::now();
        {
            FullProverImpl::Lease lease(fp->impl);
            FullProverImpl::Slot* slot = lease.slot;
            if (!slot) return K16_ERR_NO_DEVICE; // every device of the pool has been retired
            if (fp->impl->verify) {
                uint8_t ok = 0;
                rc = k16_prover_prove_mem_verified(slot->prover, wtns_values, n_values, nullptr, nullptr, out_json, cap, nullptr, nullptr, &ok);
                if (rc >= 0 && !ok) rc = FullProverImpl::REJECTED; // by the pairing check: the witness does not satisfy the circuit
            } else
                rc = k16_prover_prove_mem(slot->prover, wtns_values, n_values, nullptr, nullptr, out_json, cap, nullptr);
            rc = fp->impl->after_prove(slot, rc);
            if (rc == K16_ERR_HIP || rc == K16_ERR_NO_DEVICE) fp->impl->quarantine(slot);
        }
        if (prover_time_ms)
            *prover_time_ms = (int)std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count();
        return rc;
    } catch (const std::bad_alloc&) {
        return K16_ERR_NOMEM;
    } catch (...) {
        return K16_ERR_HIP;
    }
}

namespace {
FullProverImpl* impl_of(const void* fullprover);
} // namespace

// Verified proving behind the facade (include/k16.h): on = every pool slot builds its verification key from the zkey and
// attaches it.  All or nothing: when one slot cannot (no section 3 in the zkey), verification stays off.
extern "C" int k16_fullprover_set_verify(const void* fullprover, int on)
{
    try {
        FullProverImpl* impl = impl_of(fullprover);
        if (!impl) return K16_ERR_NO_DEVICE;
        std::lock_guard<std::mutex> lk(impl->mu);
        for (auto& s : impl->slots)
            if (s.busy) return K16_ERR_ARG; // a proof in flight: switch before the first prove, or between waves
        impl->verify = on != 0;
        int rc = K16_OK;
        for (auto& s : impl->slots) {
            if (s.dead) continue;
            if (!on) FullProverImpl::detach_vk(&s);
            else if ((rc = impl->attach_vk(&s)) != K16_OK) {
                fprintf(stderr, "k16 FullProver: no verification key could be built from %s: %s\n", impl->zkey_path.c_str(),
                        k16_last_error(s.ctx));
                log_line("ERROR", "verification asked for but the zkey carries no usable verification key");
                break;
            }
        }
        if (rc != K16_OK) {
            impl->verify = false;
            for (auto& s : impl->slots) FullProverImpl::detach_vk(&s);
        }
        return rc;
    } catch (const std::bad_alloc&) {
        return K16_ERR_NOMEM;
    } catch (...) {
        return K16_ERR_HIP;
    }
}

// k16_r1cs_match_zkey over the key FILE (mapped read-only for the comparison)
static int match_zkey_file(k16_ctx* ctx, const k16_r1cs* r, const char* zkey_path, uint32_t* mismatch)
{
    const int fd = open(zkey_path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) return K16_ERR_IO;
    struct stat st;
    void*       base = MAP_FAILED;
    if (fstat(fd, &st) == 0 && st.st_size > 0) base = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    if (base == MAP_FAILED) return K16_ERR_IO;
    const int rc = k16_r1cs_match_zkey(ctx, r, base, (size_t)st.st_size, mismatch);
    munmap(base, (size_t)st.st_size);
    return rc;
}

// Checked proving behind the facade (include/k16.h).  All or nothing, as k16_fullprover_set_verify: the circuit is compared with
// the zkey once, then every live slot gets a copy of its own; when one cannot, checking stays off.
extern "C" int k16_fullprover_set_r1cs(const void* fullprover, const char* r1cs_path)
{
    try {
        FullProverImpl* impl = impl_of(fullprover);
        if (!impl) return K16_ERR_NO_DEVICE;
        std::lock_guard<std::mutex> lk(impl->mu);
        for (auto& s : impl->slots)
            if (s.busy) return K16_ERR_ARG; // a proof in flight: switch before the first prove, or between waves
        impl->r1cs_path.clear();
        for (auto& s : impl->slots) FullProverImpl::detach_r1cs(&s);
        if (!r1cs_path) return K16_OK;
        impl->r1cs_path = r1cs_path;
        int  rc      = K16_OK;
        bool matched = false;
        for (auto& s : impl->slots) {
            if (s.dead) continue;
            if ((rc = k16_r1cs_create(s.ctx, r1cs_path, &s.r1cs)) != K16_OK) {
                fprintf(stderr, "k16 FullProver: %s: %s\n", r1cs_path, k16_last_error(s.ctx));
                if (rc == K16_ERR_IO || rc == K16_ERR_CURVE || rc == K16_ERR_ARG) rc = K16_ERR_FORMAT; // (an unusable file, whatever the reason)
                break;
            }
            if (!matched) { // once: do the circuit and the proving key belong together?
                uint32_t mismatch = 0;
                rc = match_zkey_file(s.ctx, s.r1cs, impl->zkey_path.c_str(), &mismatch);
                if (rc == K16_OK && mismatch) rc = K16_ERR_FORMAT;
                if (rc != K16_OK) {
                    fprintf(stderr, "k16 FullProver: %s is not the circuit of %s: %s\n", r1cs_path, impl->zkey_path.c_str(),
                            k16_last_error(s.ctx));
                    log_line("ERROR", "R1CS check asked for but the circuit is not the proving key's");
                    if (rc != K16_ERR_NOMEM && rc != K16_ERR_HIP) rc = K16_ERR_FORMAT;
                    break;
                }
                matched = true;
            }
            if ((rc = k16_prover_set_r1cs(s.prover, s.r1cs)) != K16_OK) {
                fprintf(stderr, "k16 FullProver: %s\n", k16_last_error(s.ctx));
                break;
            }
        }
        if (rc != K16_OK) {
            impl->r1cs_path.clear();
            for (auto& s : impl->slots) FullProverImpl::detach_r1cs(&s);
        }
        return rc;
    } catch (const std::bad_alloc&) {
        return K16_ERR_NOMEM;
    } catch (...) {
        return K16_ERR_HIP;
    }
}

extern "C" int k16_fullprover_last_rejection(uint64_t* n_failed, uint32_t* h_failed, uint32_t cap, int* status)
{
    if (!n_failed || !status) return K16_ERR_ARG;
    *status   = t_rejection.status;
    *n_failed = t_rejection.status == K16_CHECK_BROKEN ? t_rejection.n_failed : 0;
    if (h_failed)
        for (uint64_t k = 0; k < *n_failed && k < cap && k < K16_R1CS_REPORT_MAX; k++) h_failed[k] = t_rejection.lowest[k];
    return K16_OK;
}

namespace {
struct FullProverFields { // the object's two (private) fields, in the order the header -- the reference's -- declares them
    FullProverImpl* impl;
    FullProverState state;
};
FullProverImpl* impl_of(const void* fullprover)
{
    static_assert(sizeof(FullProverFields) == sizeof(FullProver), "FullProver layout");
    if (!fullprover) return nullptr;
    FullProverFields f;
    memcpy(&f, fullprover, sizeof f);
    return (f.state == FullProverState::OK) ? f.impl : nullptr;
}
} // namespace

// The compact hand-off through the pool (include/k16.h): lease a slot, hand out ITS pinned upload buffers, prove, release.
extern "C" int k16_fullprover_compact_lease(const void* fullprover, void** lease, uint8_t** narrow, uint32_t** wide_idx,
                                            uint8_t** wide_val, uint64_t* wide_cap, uint32_t* n_vars)
{
    try {
        if (!lease || !narrow || !wide_idx || !wide_val || !wide_cap) return K16_ERR_ARG;
        *lease = nullptr;
        FullProverImpl* impl = impl_of(fullprover);
        if (!impl) return K16_ERR_NO_DEVICE;
        FullProverImpl::Slot* slot = impl->acquire();
        if (!slot) return K16_ERR_NO_DEVICE;
        int rc = k16_prover_compact_buffers(slot->prover, narrow, wide_idx, wide_val, wide_cap);
        if (!rc && n_vars) rc = k16_prover_info(slot->prover, n_vars, nullptr, nullptr, nullptr);
        if (rc) {
            impl->release(slot);
            return rc;
        }
        *lease = slot;
        return K16_OK;
    } catch (const std::bad_alloc&) {
        return K16_ERR_NOMEM;
    } catch (...) {
        return K16_ERR_HIP;
    }
}

static FullProverImpl::Slot* leased_slot(FullProverImpl* impl, void* lease)
{
    if (!impl || !lease) return nullptr;
    for (auto& s : impl->slots)
        if (&s == lease) return s.busy ? &s : nullptr; // (a stale or foreign pointer never reaches a prover)
    return nullptr;
}

extern "C" int k16_fullprover_prove_compact(const void* fullprover, void* lease, uint64_t n_wide, char* out_json, size_t cap,
                                            int* prover_time_ms)
{
    try {
        if (prover_time_ms) *prover_time_ms = 0;
        FullProverImpl*       impl = impl_of(fullprover);
        FullProverImpl::Slot* slot = leased_slot(impl, lease);
        if (!slot) return K16_ERR_ARG;
        struct Release { // the slot goes back whatever happens below
            FullProverImpl*       impl;
            FullProverImpl::Slot* slot;
            ~Release() { impl->release(slot); }
        } rel{impl, slot};
        if (!out_json) return K16_ERR_ARG;
        const auto t0 = std::chrono::steady_clock::now();
        int        rc;
        if (impl->verify) {
            uint8_t ok = 0;
            rc = k16_prover_prove_compact_verified(slot->prover, n_wide, nullptr, nullptr, out_json, cap, nullptr, nullptr, &ok);
            if (rc >= 0 && !ok) rc = FullProverImpl::REJECTED; // by the pairing check: the witness does not satisfy the circuit
        } else
            rc = k16_prover_prove_compact(slot->prover, n_wide, nullptr, nullptr, out_json, cap, nullptr);
        rc = impl->after_prove(slot, rc);
        if (rc == K16_ERR_HIP || rc == K16_ERR_NO_DEVICE) impl->quarantine(slot);
        if (prover_time_ms)
            *prover_time_ms = (int)std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count();
        return rc;
    } catch (const std::bad_alloc&) {
        return K16_ERR_NOMEM;
    } catch (...) {
        return K16_ERR_HIP;
    }
}

extern "C" int k16_fullprover_compact_cancel(const void* fullprover, void* lease)
{
    try {
        FullProverImpl*       impl = impl_of(fullprover);
        FullProverImpl::Slot* slot = leased_slot(impl, lease);
        if (!slot) return K16_ERR_ARG;
        impl->release(slot);
        return K16_OK;
    } catch (...) {
        return K16_ERR_HIP;
    }
}

ProverResponse FullProver::prove(const char* input) const
{
    if (state != FullProverState::OK || !impl) return ProverResponse(ProverError::PROVER_NOT_READY);
    if (!input) return ProverResponse(ProverError::INVALID_INPUT);
    try {
        log_line("INFO", "FullProver::prove begin");
        char  json[2048];
        float dev_ms = 0;
        float prove_ms = 0;
        int   rc, dev_used = -1;
        {
            FullProverImpl::Lease lease(impl);
            FullProverImpl::Slot* slot = lease.slot;
            if (!slot) return ProverResponse(ProverError::PROVER_NOT_READY); // every device of the pool has been retired
            dev_used = slot->device;
            if (impl->verify) {
                uint8_t ok = 0;
                rc = k16_prover_prove_file_verified(slot->prover, input, nullptr, nullptr, json, sizeof json, &dev_ms, &prove_ms, nullptr, &ok);
                if (rc >= 0 && !ok) {
                    log_line("ERROR", "proof rejected by the GPU check: the witness does not satisfy the circuit");
                    rc = FullProverImpl::REJECTED; // -> INVALID_INPUT below
                }
            } else
                rc = k16_prover_prove_file_timed(slot->prover, input, nullptr, nullptr, json, sizeof json, &dev_ms, &prove_ms);
            rc = impl->after_prove(slot, rc); // (the R1CS check's finding; a rejection by either check -> INVALID_INPUT below)
            if (rc < 0 && rc != K16_ERR_CURVE && log_on())
                fprintf(stderr, "k16 FullProver::prove failed: %s\n", k16_last_error(slot->ctx));
            // A HIP failure is the DEVICE's fault, not the caller's: PROVER_NOT_READY (the service's retry / failover class,
            // RS/fullprover.cpp:117-121), and the slot goes back into the pool only after it has been rebuilt
            if (rc == K16_ERR_HIP || rc == K16_ERR_NO_DEVICE) impl->quarantine(slot);
        }
        if (rc == K16_ERR_CURVE) {
            log_line("ERROR", "witness file uses a different curve than bn128");
            return ProverResponse(ProverError::WITNESS_GENERATION_INVALID_CURVE);
        }
        if (rc == K16_ERR_HIP || rc == K16_ERR_NO_DEVICE) {
            log_line("ERROR", "device fault during prove; prover slot re-initialised");
            return ProverResponse(ProverError::PROVER_NOT_READY);
        }
        if (rc == K16_ERR_NOMEM) { // host allocation failure inside the library: the proof was cleaned up, the slot is intact
            log_line("ERROR", "out of host memory during prove");
            return ProverResponse(ProverError::PROVER_NOT_READY);
        }
        if (rc < 0) return ProverResponse(ProverError::INVALID_INPUT);
        ProverResponseMetrics m;
        // the reference's metric brackets prover->prove() only, after the witness file has been opened and checked
        // (RS/fullprover.cpp:226-231, whole milliseconds by duration_cast = truncation)
        m.prover_time = (int)prove_ms;
        if (log_on()) {
            char line[128];
            snprintf(line, sizeof line, "Time taken for Groth16 prover: %d milliseconds (device %.3f ms) on device %d",
                     m.prover_time, dev_ms, dev_used);
            log_line("INFO", line);
        }
        char* copy = strdup(json);
        if (!copy) return ProverResponse(ProverError::PROVER_NOT_READY);
        return ProverResponse(copy, m);
    } catch (...) { // std::bad_alloc / std::system_error from the pool's mutex: never across the FFI
        return ProverResponse(ProverError::PROVER_NOT_READY);
    }
}
