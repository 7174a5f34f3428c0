// msda_api.hip — library-level pieces of the C ABI: version, last-error text, A/B options.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <hip/hip_runtime.h>

#include <atomic>
#include <thread>
#include <vector>
#include <map>
#include <mutex>
#include <string>

#include "../../include/msda_hip.h"
#include "msda_options.hpp"

namespace msda {

// the options: one atomic and one getter per line of the list (msda_options.hpp)
#define MSDA_OPTION_SLOT(key, def, lo, hi, dev) \
    static std::atomic<int> g_##key{def};       \
    int option_##key() { return g_##key.load(std::memory_order_relaxed); }
MSDA_OPTION_LIST(MSDA_OPTION_SLOT)
#undef MSDA_OPTION_SLOT

// One side stream + two events per (host thread, device), created on first use and kept for the life of the thread.
// Per THREAD, because the fork (record on the user's stream, wait on the side stream) and the join are two calls
// each: with a stream / event pair shared by all callers, two threads issuing backwards on one device (autograd's
// worker threads, different user streams) could interleave record(A) record(B) wait(.) and make the sample kernel wait
// for the wrong work.  Inside one thread everything is in program order, whatever streams the caller alternates.
static const std::thread::id g_loader_thread = std::this_thread::get_id();  // the thread that loaded the library
struct SideStream {
    hipStream_t stream = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    bool tried = false;
    // a host thread that ends gives its stream and events back (thread pools, per-call worker threads); at process
    // exit the runtime may already be gone: errors are swallowed
    ~SideStream()
    {
        if (std::this_thread::get_id() == g_loader_thread) return;  // process exit: leave it to the runtime's teardown
        if (join != nullptr) (void)hipEventDestroy(join);
        if (fork != nullptr) (void)hipEventDestroy(fork);
        if (stream != nullptr) (void)hipStreamDestroy(stream);
        (void)hipGetLastError();
    }
};
static thread_local SideStream t_side[64];

static SideStream *side_for_current_device()
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    SideStream &s = t_side[dev];
    if (!s.tried) {
        s.tried = true;
        if (hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&s.fork, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&s.join, hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            s.stream = nullptr;
        }
    }
    return s.stream ? &s : nullptr;
}

hipStream_t side_stream_fork(hipStream_t user)
{
    SideStream *s = side_for_current_device();
    if (s == nullptr) return nullptr;
    if (hipEventRecord(s->fork, user) != hipSuccess || hipStreamWaitEvent(s->stream, s->fork, 0) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return s->stream;
}

int side_stream_join(hipStream_t user)
{
    SideStream *s = side_for_current_device();
    if (s == nullptr) return (int)hipErrorInvalidValue;
    hipError_t e = hipEventRecord(s->join, s->stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(user, s->join, 0);
    return (int)e;
}
static thread_local char g_err[256] = "";

// CUs of the current device, asked once per device (the LDS-level gather variants size their grid by it)
int device_cu_count()
{
    static std::atomic<int> cached[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    int n = cached[dev].load(std::memory_order_relaxed);
    if (n > 0) return n;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        n = 256;  // MI355X
    }
    cached[dev].store(n, std::memory_order_relaxed);
    return n;
}

// ---- measurement only: device time of every kernel the library launches on this thread (option "profile") ----
struct ProfileRec {
    const char *name;
    hipEvent_t a, b;
    bool ended;  // profile_end has recorded `b` (only then may msda_profile_read consume the record)
};
// (process-wide: autograd launches the backward from its own thread.  Records are heap objects and the token handed to
// the launch is the record itself, so a read that runs between a launch's begin and end can neither redirect nor drop it;
// every access to the list is under the mutex — ADVICE r04)
static std::vector<ProfileRec *> t_profile;
static std::mutex t_profile_mutex;

void *profile_begin(const char *name, hipStream_t stream)
{
    if (!option_profile()) return nullptr;
    const std::lock_guard<std::mutex> lock(t_profile_mutex);
    if (t_profile.size() >= 65536) return nullptr;
    hipEvent_t a = nullptr, b = nullptr;
    if (hipEventCreate(&a) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    if (hipEventCreate(&b) != hipSuccess || hipEventRecord(a, stream) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipEventDestroy(a);
        if (b != nullptr) (void)hipEventDestroy(b);
        return nullptr;
    }
    ProfileRec *r = new ProfileRec{name, a, b, false};
    t_profile.push_back(r);
    return r;
}

void profile_end(void *token, hipStream_t stream)
{
    if (token == nullptr) return;
    ProfileRec *r = static_cast<ProfileRec *>(token);
    const std::lock_guard<std::mutex> lock(t_profile_mutex);
    (void)hipEventRecord(r->b, stream);
    r->ended = true;
}

// ---- measurement only: what the last launches were (msda_last_launch_info) — process-wide, like the profile records:
//      autograd issues the backward from its own thread ----
constexpr int kLaunchInfoSlots = 25;  // (msda_launch.hpp, note_launch: 0-7 as before, 8-16 the instantiations, 17-22 the sorted pipeline, 23-24 the trips)
static std::atomic<int> g_info[kLaunchInfoSlots];
void note_launch(int slot, int value)
{
    if (slot >= 0 && slot < kLaunchInfoSlots) g_info[slot].store(value, std::memory_order_relaxed);
}
// ... and launches per grid form (plane_grid): counters, not last values — a route makes several plane_grid launches, and a
// test wants to know that NONE of them took another form (reported modulo 2^31)
static std::atomic<unsigned> g_grid[3];
void note_grid(int form)
{
    if (form >= 0 && form < 3) g_grid[form].fetch_add(1u, std::memory_order_relaxed);
}

void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

}  // namespace msda

extern "C" int msda_abi_version(void) { return MSDA_ABI_VERSION; }

extern "C" const char *msda_last_error(void) { return msda::g_err; }

extern "C" int msda_last_launch_info(const char *key)
{
    static const char *const kKeys[msda::kLaunchInfoSlots] = {
        "fwd_variant", "fwd_lds_level_bytes", "fwd_lds_planes", "fwd_workgroups", "sample_variant", "sample_lds_level_bytes",
        "value_path", "value_passes",
        // the template instantiation of the last forward / sample-gradient / grad_value launch (note_instance)
        "fwd_vec", "fwd_group", "fwd_chunks", "sample_vec", "sample_group", "sample_chunks", "value_vec", "value_group",
        "value_chunks",
        // the sorted grad_value pipeline's table sizes, place-pass variant, query slices, rounds and gather window
        "value_cell_cap", "value_place_cells", "value_place_variant", "value_slices", "value_rounds", "value_win",
        // passes over a unit's samples of the last forward / sample-gradient launch (note_trips)
        "fwd_trips", "sample_trips"};
    for (int i = 0; key != nullptr && i < msda::kLaunchInfoSlots; ++i)
        if (strcmp(key, kKeys[i]) == 0) return msda::g_info[i].load(std::memory_order_relaxed);
    static const char *const kGridKeys[3] = {"grid_xcd3d_launches", "grid_linear2d_launches", "grid_flat_launches"};
    for (int i = 0; key != nullptr && i < 3; ++i)
        if (strcmp(key, kGridKeys[i]) == 0) return (int)(msda::g_grid[i].load(std::memory_order_relaxed) & 0x7fffffffu);
    msda::set_error("unknown launch-info key '%s'", key ? key : "(null)");
    return MSDA_ERR_BAD_ARG;
}

// "name launches total_us\n" per kernel launched on this thread since the last read while option "profile" was 1;
// (any thread: the records are process-wide) waits for the recorded events, then forgets them.  Returns the number of characters written (without the NUL).
extern "C" int msda_profile_read(char *buf, int cap)
{
    std::map<std::string, std::pair<int, double>> acc;
    const std::lock_guard<std::mutex> lock(msda::t_profile_mutex);
    std::vector<msda::ProfileRec *> open;  // begun, not ended yet: they stay for the next read
    for (msda::ProfileRec *r : msda::t_profile) {
        if (!r->ended) {
            open.push_back(r);
            continue;
        }
        float ms = 0.f;
        if (hipEventSynchronize(r->b) == hipSuccess && hipEventElapsedTime(&ms, r->a, r->b) == hipSuccess) {
            auto &e = acc[r->name];
            e.first += 1;
            e.second += (double)ms * 1e3;
        }
        (void)hipEventDestroy(r->a);
        (void)hipEventDestroy(r->b);
        delete r;
    }
    (void)hipGetLastError();
    msda::t_profile.swap(open);
    std::string out;
    for (const auto &kv : acc) {
        char line[160];
        snprintf(line, sizeof(line), "%s %d %.3f\n", kv.first.c_str(), kv.second.first, kv.second.second);
        out += line;
    }
    if (buf == nullptr || cap <= 0) return (int)out.size();
    const int n = (int)out.size() < cap - 1 ? (int)out.size() : cap - 1;
    memcpy(buf, out.data(), (size_t)n);
    buf[n] = 0;
    return n;
}

// One table for set and get, made from the option list (msda_options.hpp).  dev: an experiment knob, reachable only in builds with -DMSDA_DEV (include/msda_hip.h).
namespace msda {
struct OptionEntry {
    const char *key;
    std::atomic<int> *slot;
    int lo, hi;  // accepted range (values outside are rejected)
    bool dev;
};
static const OptionEntry kOptions[] = {
#define MSDA_OPTION_ROW(key, def, lo, hi, dev) {#key, &g_##key, lo, hi, dev},
    MSDA_OPTION_LIST(MSDA_OPTION_ROW)
#undef MSDA_OPTION_ROW
};
static const OptionEntry *find_option(const char *key)
{
    if (key == nullptr) return nullptr;
    for (const OptionEntry &o : kOptions) {
        if (strcmp(key, o.key) != 0) continue;
#ifndef MSDA_DEV
        if (o.dev) return nullptr;
#endif
        return &o;
    }
    return nullptr;
}
}  // namespace msda

extern "C" int msda_set_option(const char *key, int value)
{
    const msda::OptionEntry *o = msda::find_option(key);
    if (o == nullptr) {
        msda::set_error("unknown option '%s'", key ? key : "(null)");
        return MSDA_ERR_BAD_ARG;
    }
    if (value < o->lo || value > o->hi || (o->slot == &msda::g_value_path && value == 1) ||
        (o->slot == &msda::g_gather_win && value != 0 && value < 8)) {
        msda::set_error("option '%s': value %d out of range [%d, %d]", key, value, o->lo, o->hi);
        return MSDA_ERR_BAD_ARG;
    }
    o->slot->store(value, std::memory_order_relaxed);
    return 0;
}

extern "C" int msda_get_option(const char *key)
{
    const msda::OptionEntry *o = msda::find_option(key);
    if (o == nullptr) {
        msda::set_error("unknown option '%s'", key ? key : "(null)");
        return MSDA_ERR_BAD_ARG;
    }
    return o->slot->load(std::memory_order_relaxed);
}
