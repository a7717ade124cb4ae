// host_runtime.hip -- the library's host runtime, shared by every operator: the error text, the stage timers, the host marks of
// r2_profile_host, the pinned read-back words and the mailbox, the defer slot pool and the per-device queries.  Host code only: no
// kernel lives here (declarations: r2_common.hpp).
#include "r2_common.hpp"
#include <chrono>
#include <mutex>
#include <cstdlib>
#include <cstring>
#include <stdarg.h>
#include <vector>
#include <string.h>

namespace r2 {

static thread_local char g_err[512] = "";
void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
const char *get_error() { return g_err; }

// ---- stage timers: event pairs recorded on the caller's stream, resolved lazily in r2_profile_read
int g_profile_mask_on = 0;
static unsigned long long g_profile_mask = 0;
struct Pending { int stage; hipEvent_t a, b; };
static std::vector<Pending> g_pending;
static std::vector<hipEvent_t> g_pool;
static hipEvent_t g_open[ST_COUNT];
static double g_ms[ST_COUNT];
static long long g_cnt[ST_COUNT];
static const char *const g_stage_names[ST_COUNT] = {
    "raster.preprocess", "raster.scan", "raster.duplicate", "raster.sort", "raster.ranges", "raster.render_fwd",
    "raster.render_bwd", "raster.geom_bwd", "voxel.preprocess", "voxel.scan", "voxel.duplicate", "voxel.sort",
    "voxel.ranges", "voxel.render_fwd", "voxel.render_bwd", "voxel.geom_bwd", "knn.dist2", "raster.depth_sort",
    "voxel.depth_sort"};

static hipEvent_t pool_get()
{
    if (!g_pool.empty()) { hipEvent_t e = g_pool.back(); g_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}
void stage_begin(int stage, hipStream_t s)
{
    if (!((g_profile_mask >> stage) & 1ull)) return;
    hipEvent_t e = pool_get();
    (void)hipEventRecord(e, s);
    g_open[stage] = e;
}
void stage_end(int stage, hipStream_t s)
{
    if (!((g_profile_mask >> stage) & 1ull)) return;
    hipEvent_t e = pool_get();
    (void)hipEventRecord(e, s);
    g_pending.push_back({stage, g_open[stage], e});
}

static double g_sync_wait_us = 0.0;
static long long g_sync_calls = 0;
// host time of the forward passes around their synchronisation point (r2_profile_host)
static double g_pre_sync_us = 0.0, g_post_sync_us = 0.0;
static long long g_fwd_calls = 0;
static thread_local std::chrono::steady_clock::time_point g_fwd_t0, g_fwd_t1;
void host_mark_forward_begin() { g_fwd_t0 = std::chrono::steady_clock::now(); }
void host_mark_wait_begin() { g_pre_sync_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - g_fwd_t0).count(); }
void host_mark_wait_end() { g_fwd_t1 = std::chrono::steady_clock::now(); }
void host_mark_forward_end()
{
    g_post_sync_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - g_fwd_t1).count();
    g_fwd_calls += 1;
}

// pinned destination (pageable ones are staged and synchronised by the runtime) and a busy-wait on an event: the GPU is
// idle until the host has seen these words and launched the rest of the forward pass, so wake-up latency is on the
// critical path -- a blocking hipStreamSynchronize may sleep on an interrupt (tens of microseconds)
// pinned host words of the calling thread (the device -> host read-back and the mailbox below): released when the thread exits
struct PinnedWords {
    uint32_t *p = nullptr;
    void release() { if (p) { if (hipHostFree(p) != hipSuccess) (void)hipGetLastError(); p = nullptr; } }
    ~PinnedWords() { release(); }
};
static thread_local PinnedWords g_pinned_holder, g_mailbox_holder;
#define g_pinned g_pinned_holder.p
// one event per device: an event can only be recorded on a stream of the device it was created on, and one host thread may
// drive several GPUs (the caller makes the stream's device current, like every HIP API that takes a stream)
constexpr int MAX_DEVICES = R2_MAX_DEVICES;
static thread_local hipEvent_t g_read_evs[MAX_DEVICES] = {};
static thread_local hipEvent_t g_read_ev = nullptr;   // the event of the read in flight

int current_device_slot()
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) dev = 0;
    return dev % MAX_DEVICES;
}

// A kernel that needs more than the default 64 KB of dynamic LDS has to be told so once PER DEVICE (a host thread may drive several
// GPUs): state[] is the call site's table (0 = not asked yet, 1 = granted, -1 = refused), indexed by current_device_slot().
bool allow_dynamic_lds(const void *kernel, int bytes, signed char *state)
{
    signed char &st = state[current_device_slot()];   // written with the same value by whoever gets here first: a benign race
    if (st == 0) {
        if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess) st = 1;
        else { (void)hipGetLastError(); st = -1; }
    }
    return st > 0;
}

size_t device_lds_optin_bytes()
{
    static size_t lim[MAX_DEVICES] = {};   // written once per device with the same value
    const int slot = current_device_slot();
    if (lim[slot] == 0) {
        int dev = 0, a = 0, b = 0;
        if (hipGetDevice(&dev) != hipSuccess) (void)hipGetLastError();
        // runtimes differ in which of the two attributes carries the opt-in limit (gfx950: 160 KB): take the larger
        if (hipDeviceGetAttribute(&a, hipDeviceAttributeSharedMemPerBlockOptin, dev) != hipSuccess) { (void)hipGetLastError(); a = 0; }
        if (hipDeviceGetAttribute(&b, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) { (void)hipGetLastError(); b = 0; }
        const int n = std::max(std::max(a, b), 64 * 1024);   // 64 KB: what every device grants without asking
        lim[slot] = (size_t)n;
    }
    return lim[slot];
}

int device_cu_count()
{
    static int cus[MAX_DEVICES] = {};   // written once per device with the same value: a benign race at worst
    const int slot = current_device_slot();
    if (cus[slot] == 0) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
            n = 256;
        cus[slot] = n;
    }
    return cus[slot];
}

int read_host_words_begin(const uint32_t *dev_words, int n, hipStream_t s)
{
    if (n < 1 || n > 16) {
        set_error("read_host_words: %d words", n);
        return R2_ERR_INVALID;
    }
    if (!g_pinned) R2_HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&g_pinned), 64, hipHostMallocPortable));
    hipEvent_t &ev = g_read_evs[current_device_slot()];
    if (!ev) R2_HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    g_read_ev = ev;
    R2_HIP_TRY(hipMemcpyAsync(g_pinned, dev_words, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    R2_HIP_TRY(hipEventRecord(g_read_ev, s));
    return 0;
}

int read_host_words_wait(uint32_t *out, int n)
{
    hipError_t q;
    host_mark_wait_begin();
    const auto t0 = std::chrono::steady_clock::now();
    while ((q = hipEventQuery(g_read_ev)) == hipErrorNotReady) __builtin_ia32_pause();
    g_sync_wait_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    g_sync_calls += 1;
    host_mark_wait_end();
    if (q != hipSuccess) {
        set_error("read_host_words: %s", hipGetErrorString(q));
        return -(int)q;
    }
    for (int i = 0; i < n; ++i) out[i] = g_pinned[i];
    return 0;
}

// Zero-copy variant for the hinted forward path: the kernel that produces the last of the words stores them, then a
// sequence number (release, system scope), straight into pinned host memory, and the host spins on the sequence number.
// No copy kernel (4 us of stream time on this runtime + a ~5 us signalling gap behind it) and no event.
#define g_mailbox g_mailbox_holder.p   // [16]: words 0..14, sequence number at 15
static thread_local uint32_t g_mailbox_seq = 0;

int host_mailbox_arm(uint32_t **mailbox, uint32_t *seq)
{
    if (!g_mailbox) {
        R2_HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&g_mailbox), 64,
                                 hipHostMallocPortable | hipHostMallocMapped | hipHostMallocCoherent));
        memset(g_mailbox, 0, 64);
    }
    if (++g_mailbox_seq == 0u) ++g_mailbox_seq;   // 0 = never written
    *mailbox = g_mailbox;
    *seq = g_mailbox_seq;
    return 0;
}

void host_words_release() { g_pinned_holder.release(); g_mailbox_holder.release(); }

static int mailbox_spin(uint32_t *words, uint32_t seq, uint32_t *out, int n, hipStream_t s);
int host_mailbox_wait(uint32_t seq, uint32_t *out, int n, hipStream_t s) { return mailbox_spin(g_mailbox, seq, out, n, s); }

static int mailbox_spin(uint32_t *words, uint32_t seq, uint32_t *out, int n, hipStream_t s)
{
    host_mark_wait_begin();
    const auto t0 = std::chrono::steady_clock::now();
    volatile uint32_t *mb = words;
    unsigned spins = 0;
    bool drained = false;
    static const double timeout_s = [] { const char *e = getenv("R2_SYNC_TIMEOUT_S"); const double v = e ? atof(e) : 0.0; return v > 0.0 ? v : 30.0; }();
    while (__atomic_load_n(&words[15], __ATOMIC_ACQUIRE) != seq) {
        __builtin_ia32_pause();
        if ((++spins & 0x3FFFu) == 0u) {   // the producing kernel never ran?  (launch failure: do not spin forever)
            // a hung GPU or a stream blocked on something that never happens: give up after a wall-clock limit instead of
            // spinning forever (R2_SYNC_TIMEOUT_S, default 30 s); kernels queued so far may still write the mailbox later,
            // which is harmless -- the next call uses a new sequence number
            if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_s) {
                set_error("host_mailbox_wait: no control words from the GPU after %.0f s (hung device or blocked stream)", timeout_s);
                return R2_ERR_INVALID;
            }
            const hipError_t q = hipStreamQuery(s);
            if (q != hipSuccess && q != hipErrorNotReady) {
                set_error("host_mailbox_wait: %s", hipGetErrorString(q));
                return -(int)q;
            }
            if (q == hipSuccess) {
                if (drained) {
                    set_error("host_mailbox_wait: stream drained without the forward's control words arriving");
                    return R2_ERR_INVALID;
                }
                drained = true;
            }
        }
    }
    g_sync_wait_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    g_sync_calls += 1;
    host_mark_wait_end();
    for (int i = 0; i < n; ++i) out[i] = mb[i];
    return 0;
}

// ---- deferred num_rendered (round 6; r2_defer_count_control).  A forward that does not wait for its control words leaves them in a
// SLOT of a small process-wide pool of pinned words and returns a token naming the slot; whoever calls the matching backward -- with
// torch that is the autograd engine's thread, not the forward's -- resolves the token there: by then the forward's second kernel
// has long posted the words, so the wait that cost the forward ~95 of its 170 us of host time is gone, not moved.
// Slots are handed out by one mutex-protected table; a slot whose forward has completed but whose backward never came (rendering
// under no_grad) is recycled, least recently used first.
namespace {
constexpr int DEFER_SLOTS = 64;
struct DeferSlot { uint32_t seq = 0; uint32_t cap = 0; bool busy = false; bool short_seen = false; unsigned long long used = 0; };
std::mutex g_defer_mu;
uint32_t *g_defer_words = nullptr;   // [DEFER_SLOTS][16] pinned, never freed (process lifetime: tokens may outlive any thread)
DeferSlot g_defer[DEFER_SLOTS];
uint32_t g_defer_seq = 0;
unsigned long long g_defer_tick = 0;
}  // namespace

int defer_acquire(uint32_t **mailbox, uint32_t *seq, uint32_t cap)
{
    std::lock_guard<std::mutex> lk(g_defer_mu);
    if (!g_defer_words) {
        if (hipHostMalloc(reinterpret_cast<void **>(&g_defer_words), DEFER_SLOTS * 64,
                          hipHostMallocPortable | hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {
            (void)hipGetLastError();
            g_defer_words = nullptr;
            return -1;
        }
        memset(g_defer_words, 0, DEFER_SLOTS * 64);
    }
    int pick = -1;
    for (int i = 0; i < DEFER_SLOTS && pick < 0; ++i)
        if (!g_defer[i].busy) pick = i;
    if (pick < 0) {   // every slot is waiting for a backward: recycle the oldest one whose forward has posted its words
        for (int i = 0; i < DEFER_SLOTS; ++i)
            if (__atomic_load_n(&g_defer_words[i * 16 + 15], __ATOMIC_ACQUIRE) == g_defer[i].seq &&
                (pick < 0 || g_defer[i].used < g_defer[pick].used))
                pick = i;
        if (pick < 0) return -1;   // none: the caller falls back to the waiting forward
    }
    if (++g_defer_seq == 0u) ++g_defer_seq;
    g_defer[pick] = DeferSlot{g_defer_seq, cap, true, false, ++g_defer_tick};
    *mailbox = g_defer_words + pick * 16;
    *seq = g_defer_seq;
    return DEFER_TOKEN_FLAG | (pick << 16) | (int)(g_defer_seq & 0xFFFFu);
}

// -> 0 and the words, or an error: the token is stale (its slot was recycled), or the device never posted
int defer_resolve(int token, uint32_t *out, int n, uint32_t *cap, hipStream_t s, bool release)
{
    const int slot = (token >> 16) & (DEFER_SLOTS - 1);
    uint32_t seq = 0;
    {
        std::lock_guard<std::mutex> lk(g_defer_mu);
        if (!g_defer_words || !g_defer[slot].busy || (g_defer[slot].seq & 0xFFFFu) != (uint32_t)(token & 0xFFFF)) {
            set_error("deferred num_rendered: stale token (the forward's slot was recycled: more than %d forwards without a backward)",
                      DEFER_SLOTS);
            return R2_ERR_INVALID;
        }
        seq = g_defer[slot].seq;
        if (cap) *cap = g_defer[slot].cap;
    }
    const int rc = mailbox_spin(g_defer_words + slot * 16, seq, out, n, s);
    if (release) {
        std::lock_guard<std::mutex> lk(g_defer_mu);
        if (g_defer[slot].seq == seq) g_defer[slot].busy = false;
    }
    return rc;
}

// non-blocking: have the words of this token arrived?  (the forward's own thread keeps its predictions current with it) -> the
// words and the capacity the forward was launched with
bool defer_peek(int token, uint32_t *out, int n, uint32_t *cap)
{
    const int slot = (token >> 16) & (DEFER_SLOTS - 1);
    std::lock_guard<std::mutex> lk(g_defer_mu);
    if (!g_defer_words || (g_defer[slot].seq & 0xFFFFu) != (uint32_t)(token & 0xFFFF)) return false;
    uint32_t *w = g_defer_words + slot * 16;
    if (__atomic_load_n(&w[15], __ATOMIC_ACQUIRE) != g_defer[slot].seq) return false;
    for (int i = 0; i < n; ++i) out[i] = w[i];
    *cap = g_defer[slot].cap;
    return true;
}

// true the first time it is called for a token (of the slot's current forward): a short count is reported once per forward,
// whoever finds it first
bool defer_first_short(int token)
{
    const int slot = (token >> 16) & (DEFER_SLOTS - 1);
    std::lock_guard<std::mutex> lk(g_defer_mu);
    if ((g_defer[slot].seq & 0xFFFFu) != (uint32_t)(token & 0xFFFF) || g_defer[slot].short_seen) return false;
    g_defer[slot].short_seen = true;
    return true;
}

int read_host_words(const uint32_t *dev_words, uint32_t *out, int n, hipStream_t s)
{
    const int rc = read_host_words_begin(dev_words, n, s);
    return rc ? rc : read_host_words_wait(out, n);
}

}  // namespace r2

extern "C" const char *r2_last_error(void) { return r2::get_error(); }

extern "C" int r2_abi_version(void) { return R2_ABI_VERSION; }

extern "C" int r2_sync_wait_stats(double *total_us, long long *calls, int reset)
{
    if (total_us) *total_us = r2::g_sync_wait_us;
    if (calls) *calls = r2::g_sync_calls;
    if (reset) { r2::g_sync_wait_us = 0.0; r2::g_sync_calls = 0; }
    return 0;
}

extern "C" int r2_profile_host(double *pre_sync_us, double *post_sync_us, long long *calls, int reset)
{
    if (pre_sync_us) *pre_sync_us = r2::g_pre_sync_us;
    if (post_sync_us) *post_sync_us = r2::g_post_sync_us;
    if (calls) *calls = r2::g_fwd_calls;
    if (reset) { r2::g_pre_sync_us = r2::g_post_sync_us = 0.0; r2::g_fwd_calls = 0; }
    return 0;
}

extern "C" void r2_profile_enable(unsigned long long stage_mask)
{
    r2::g_profile_mask = stage_mask;
    r2::g_profile_mask_on = stage_mask != 0;
}
extern "C" int r2_profile_stage_count(void) { return r2::ST_COUNT; }
extern "C" const char *r2_profile_stage_name(int stage)
{
    return (stage >= 0 && stage < r2::ST_COUNT) ? r2::g_stage_names[stage] : "";
}
extern "C" int r2_profile_read(double *total_ms, long long *counts, int reset)
{
    using namespace r2;
    for (auto &p : g_pending) {
        float ms = 0.f;
        if (hipEventSynchronize(p.b) == hipSuccess && hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            g_ms[p.stage] += ms;
            g_cnt[p.stage] += 1;
        }
        g_pool.push_back(p.a);
        g_pool.push_back(p.b);
    }
    g_pending.clear();
    for (int i = 0; i < ST_COUNT; ++i) {
        if (total_ms) total_ms[i] = g_ms[i];
        if (counts) counts[i] = g_cnt[i];
    }
    if (reset) { memset(g_ms, 0, sizeof(g_ms)); memset(g_cnt, 0, sizeof(g_cnt)); }
    return ST_COUNT;
}
