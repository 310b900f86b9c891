// lvk_context.hip — process and context plumbing of liblvk_hip.so, used by the front-end, the filter, the stage entries and every
// test: the error text and the scratch slots of a context, the BAR self-test (lvk_bar_usable), lvk_runtime_env with the core and
// NUMA binding, lvk_context_create / destroy / set_stream, and lvk_sync / malloc / free / memcpy_* / memset.
#include "lvk_internal.h"
#include <atomic>
#include <sched.h>
#include <stdarg.h>
#include <new>
#include <vector>

lvk_status lvk_set_error(lvk_context* ctx, lvk_status code, const char* fmt, ...)
{
    if (ctx) {
        va_list ap; va_start(ap, fmt);
        vsnprintf(ctx->err, sizeof ctx->err, fmt, ap);
        va_end(ap);
    }
    return code;
}

void* lvk_ctx_scratch(lvk_context* ctx, int slot, size_t bytes)
{
    if (slot < 0 || slot >= LVK_SCRATCH_SLOTS) return nullptr;
    if (ctx->scratch_bytes[slot] >= bytes && ctx->scratch[slot]) return ctx->scratch[slot];
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) return nullptr;
    if (ctx->scratch[slot]) hipFree(ctx->scratch[slot]);
    ctx->scratch[slot] = nullptr; ctx->scratch_bytes[slot] = 0;
    if (hipMalloc(&ctx->scratch[slot], bytes) != hipSuccess) return nullptr;
    ctx->scratch_bytes[slot] = bytes;
    return ctx->scratch[slot];
}

// =========================================================================== runtime environment, BAR self-test
// plain loads, as the product kernels do them
__global__ void k_bar_probe(const unsigned* __restrict__ src, unsigned* __restrict__ dst, int n, int stride)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[(size_t)i * stride];
}
static bool bar_selftest(int device)
{
    int large_bar = 0;
    if (hipDeviceGetAttribute(&large_bar, hipDeviceAttributeIsLargeBar, device) != hipSuccess || !large_bar) { (void)hipGetLastError(); return false; }
    int prev = -1; (void)hipGetDevice(&prev);
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return false; }
    const int n = 256, stride = 64;                          // 256 words, one per 256-byte line, over 64 KB
    unsigned* d = nullptr; unsigned* h = nullptr; unsigned* dh = nullptr; hipStream_t st = nullptr;
    bool ok = hipExtMallocWithFlags((void**)&d, sizeof(unsigned) * n * stride, hipDeviceMallocFinegrained) == hipSuccess && d;
    ok = ok && hipHostMalloc((void**)&h, sizeof(unsigned) * n) == hipSuccess && hipHostGetDevicePointer((void**)&dh, h, 0) == hipSuccess;
    ok = ok && hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess;
    if (ok) {
        bool writable = false;
        if (FILE* f = fopen("/proc/self/maps", "r")) {
            char line[512]; unsigned long lo = 0, hi = 0; char perm[8] = {0};
            while (fgets(line, sizeof line, f))
                if (sscanf(line, "%lx-%lx %7s", &lo, &hi, perm) == 3 && (unsigned long)d >= lo && (unsigned long)d < hi) { writable = perm[0] == 'r' && perm[1] == 'w'; break; }
            fclose(f);
        }
        ok = writable;
    }
    for (int round = 0; round < 6 && ok; ++round) {           // the same addresses rewritten before every launch, as the filter's arena is every frame
        volatile unsigned* w = (volatile unsigned*)d;
        for (int i = 0; i < n; ++i) w[(size_t)i * stride] = 0x9e3779b9u * (unsigned)(round + 1) + (unsigned)i;
        LVK_STORE_FENCE();
        memset(h, 0, sizeof(unsigned) * n);
        hipLaunchKernelGGL(k_bar_probe, dim3(n / 64), dim3(64), 0, st, (const unsigned*)d, dh, n, stride);
        ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
        for (int i = 0; i < n && ok; ++i) ok = h[i] == 0x9e3779b9u * (unsigned)(round + 1) + (unsigned)i;
    }
    if (st) hipStreamDestroy(st);
    if (h) hipHostFree(h);
    if (d) hipFree(d);
    (void)hipGetLastError();
    if (prev >= 0 && prev != device) (void)hipSetDevice(prev);
    return ok;
}
bool lvk_bar_usable(int device)
{
    static std::atomic<int> verdict[64];                     // 0 unknown, 1 usable, 2 not
    if (device < 0 || device >= 64) return false;
    int v = verdict[device].load(std::memory_order_acquire);
    if (v == 0) {
        const char* sw = getenv("LVK_BAR_PUSH");
        bool ok = !(sw && !strcmp(sw, "0"));
        if (ok) ok = bar_selftest(device);
        else if (getenv("LVK_VERBOSE")) fprintf(stderr, "[lvk] LVK_BAR_PUSH=0: staging through pinned host memory\n");
        if (!ok && !(sw && !strcmp(sw, "0")) && getenv("LVK_VERBOSE")) fprintf(stderr, "[lvk] device %d: BAR push not usable (no large BAR, no writable mapping, or stale reads in the self-test): pinned host staging\n", device);
        v = ok ? 1 : 2;
        verdict[device].store(v, std::memory_order_release);
    }
    return v == 1;
}

// lvk_runtime_env (include/lvk_c.h): what a deployment should set before the HIP runtime initialises, done by the library.
//  * GPU_MAX_HW_QUEUES=8: the front-end's three streams + the filter's (+ the application's own) each get a hardware queue; with HIP's
//    default of 4, streams share queues and serialise (measured: 5800 -> 4800 frames/s; round 6's pipeline: 10,100 -> 7,300).  An application that asks for it by name
//    (an explicit lvk_runtime_env call with LVK_RT_HW_QUEUES) also gets a preset number below 8 raised to 8 - a launcher's or a
//    machine's blanket default of 4 would otherwise turn the request into nothing without a word; 8 or more is left alone, and
//    nothing above 8 is ever written.
//  * HIP_FORCE_DEV_KERNARG=1: kernel arguments in device memory (~1 % on these chains of small kernels).
//  * LVK_RT_BIND_L3 (opt-in: a library should not move its caller's threads unasked): the calling thread - and every thread it
//    starts afterwards: the HIP runtime's, the filter's worker - onto the physical cores of ONE L3 group of the socket it runs on
//    (rank r takes the r-th group): the caller's and the filter's thread hand each other messages every ~100 us.
// Otherwise variables the user has set are left alone: the implicit call below never overrides one.  Effective only if called before the process's first HIP call; lvk_context_create
// calls it with LVK_RT_DEFAULT itself (LVK_RUNTIME_ENV=0 turns that off), which is early enough when the library makes that first call.
static bool cpulist_parse(const char* path, cpu_set_t* out)
{
    CPU_ZERO(out);
    FILE* f = fopen(path, "r");
    if (!f) return false;
    char list[4096] = {0};
    const bool got = fgets(list, sizeof list, f) != nullptr;
    fclose(f);
    if (!got) return false;
    for (char* p = list; *p && *p != '\n';) {
        char* end = nullptr;
        long a = strtol(p, &end, 10); if (end == p) break;
        long b = a; p = end;
        if (*p == '-') { b = strtol(p + 1, &end, 10); p = end; }
        for (long c = a; c <= b && c < CPU_SETSIZE; ++c) CPU_SET((int)c, out);
        if (*p == ',') ++p;
    }
    return true;
}
static bool bind_l3_group(int local_rank)
{
    cpu_set_t allowed;
    if (sched_getaffinity(0, sizeof allowed, &allowed) != 0) return false;
    const int cpu = sched_getcpu();
    if (cpu < 0) return false;
    char path[160]; cpu_set_t node; bool have_node = false;
    for (int nd = 0; nd < 64 && !have_node; ++nd) {
        snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", nd);
        if (!cpulist_parse(path, &node)) break;
        have_node = CPU_ISSET(cpu, &node);
    }
    if (!have_node) return false;
    // one logical CPU per physical core, grouped by L3; groups in ascending order of their first CPU
    std::vector<std::pair<int, cpu_set_t>> groups;
    for (int c = 0; c < CPU_SETSIZE; ++c) {
        if (!CPU_ISSET(c, &node) || !CPU_ISSET(c, &allowed)) continue;
        cpu_set_t l3, sib;
        snprintf(path, sizeof path, "/sys/devices/system/cpu/cpu%d/cache/index3/shared_cpu_list", c);
        if (!cpulist_parse(path, &l3)) return false;
        snprintf(path, sizeof path, "/sys/devices/system/cpu/cpu%d/topology/thread_siblings_list", c);
        if (!cpulist_parse(path, &sib)) return false;
        int first_sib = -1, first_l3 = -1;
        for (int k = 0; k < CPU_SETSIZE && (first_sib < 0 || first_l3 < 0); ++k) { if (first_sib < 0 && CPU_ISSET(k, &sib)) first_sib = k; if (first_l3 < 0 && CPU_ISSET(k, &l3)) first_l3 = k; }
        if (c != first_sib) continue;
        size_t g = 0; while (g < groups.size() && groups[g].first != first_l3) ++g;
        if (g == groups.size()) { cpu_set_t z; CPU_ZERO(&z); groups.push_back(std::make_pair(first_l3, z)); }
        CPU_SET(c, &groups[g].second);
    }
    std::vector<cpu_set_t> usable;
    for (auto& g : groups) if (CPU_COUNT(&g.second) >= 4) usable.push_back(g.second);
    if (usable.empty()) return false;
    const cpu_set_t& pick = usable[(size_t)(local_rank < 0 ? 0 : local_rank) % usable.size()];
    return sched_setaffinity(0, sizeof pick, &pick) == 0;
}

// =========================================================================== context
extern "C" {

static std::atomic<bool> g_hip_touched{false};          // this library has made a HIP call in this process: the runtime has read its environment
// asked: the application called lvk_runtime_env itself (it may raise a preset GPU_MAX_HW_QUEUES below 8); the implicit call of lvk_context_create may not
static unsigned runtime_env_apply(unsigned flags, int local_rank, bool asked)
{
    unsigned done = 0;
    // a flag is reported only if it can still take effect: the variable was not set by the user and the runtime has not been
    // initialised through this library (a host application that initialised HIP itself is beyond what can be seen from here:
    // lvk_c.h says "call it first in main()")
    const bool early = !g_hip_touched.load();
    if ((flags & LVK_RT_HW_QUEUES) && early) {
        const char* cur = getenv("GPU_MAX_HW_QUEUES");
        bool set8 = !cur;
        if (cur && asked) { char* end = nullptr; const long v = strtol(cur, &end, 10); set8 = end != cur && *end == 0 && v < 8; }    // a number below 8; anything else stays
        if (set8 && setenv("GPU_MAX_HW_QUEUES", "8", 1) == 0) done |= LVK_RT_HW_QUEUES;
    }
    if ((flags & LVK_RT_DEV_KERNARG) && early && !getenv("HIP_FORCE_DEV_KERNARG")) { if (setenv("HIP_FORCE_DEV_KERNARG", "1", 0) == 0) done |= LVK_RT_DEV_KERNARG; }
    if (flags & LVK_RT_BIND_L3) { if (bind_l3_group(local_rank)) done |= LVK_RT_BIND_L3; }
    return done;
}
unsigned lvk_runtime_env(unsigned flags, int local_rank) { return runtime_env_apply(flags, local_rank, true); }

const char* lvk_version(void) { return "lvk-hip 0.1 (gfx950)"; }

// Optional placement help for dual-socket hosts (LVK_NUMA_BIND=1): restrict the thread that creates a context (and the threads it
// starts later: the pipelined filter's worker) to the CPUs of the device's NUMA node.  Off by default: a library should not move
// its caller's threads, and on the 2 x EPYC 9575F boxes measured here the node itself made no difference — what did was having
// the WHOLE process (HIP runtime initialisation included) on one socket, which is the launcher's business (bench.py does it,
// INTEGRATION.md says how: taskset / numactl).
static void bind_thread_to_device_node(int device)
{
    const char* on = getenv("LVK_NUMA_BIND");
    if (!(on && !strcmp(on, "1"))) return;
    int node = -1;
    if (hipDeviceGetAttribute(&node, hipDeviceAttributeHostNumaId, device) != hipSuccess) { (void)hipGetLastError(); node = -1; }
    char path[160];
    if (node < 0) {                                         // older runtimes: ask sysfs through the PCI address
        char bdf[32] = {0};
        if (hipDeviceGetPCIBusId(bdf, (int)sizeof bdf, device) != hipSuccess) { (void)hipGetLastError(); return; }
        for (char* c = bdf; *c; ++c) if (*c >= 'A' && *c <= 'F') *c = (char)(*c - 'A' + 'a');
        snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bdf);
        if (FILE* f = fopen(path, "r")) { if (fscanf(f, "%d", &node) != 1) node = -1; fclose(f); }
        if (node < 0) return;
    }
    snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", node);
    FILE* f = fopen(path, "r");
    if (!f) return;
    char list[1024] = {0};
    const bool got = fgets(list, sizeof list, f) != nullptr;
    fclose(f);
    if (!got) return;
    cpu_set_t allowed, want; CPU_ZERO(&allowed); CPU_ZERO(&want);
    if (sched_getaffinity(0, sizeof allowed, &allowed) != 0) return;
    int n_want = 0;
    for (char* p = list; *p && *p != '\n';) {               // "0-63,128-191"
        char* end = nullptr;
        long a = strtol(p, &end, 10); if (end == p) break;
        long b = a; p = end;
        if (*p == '-') { b = strtol(p + 1, &end, 10); p = end; }
        for (long c = a; c <= b && c < CPU_SETSIZE; ++c) if (CPU_ISSET((int)c, &allowed)) { CPU_SET((int)c, &want); ++n_want; }
        if (*p == ',') ++p;
    }
    if (n_want > 0) sched_setaffinity(0, sizeof want, &want);
}

lvk_status lvk_context_create(int device, lvk_context** out)
{
    if (!out) return LVK_ERR_ARG;
    {   // the library's runtime settings, in case this is the process's first HIP call (see lvk_runtime_env)
        static std::atomic<bool> once{false};
        if (!once.exchange(true)) { const char* sw = getenv("LVK_RUNTIME_ENV"); if (!(sw && !strcmp(sw, "0"))) {
            const char* bd = getenv("LVK_RUNTIME_BIND");               // "l3" or "l3:<local rank>": the opt-in core binding for a driver that cannot call lvk_runtime_env (the reference's own main())
            const bool l3 = bd && !strncmp(bd, "l3", 2);
            runtime_env_apply(LVK_RT_DEFAULT | (l3 ? LVK_RT_BIND_L3 : 0u), l3 && bd[2] == ':' ? atoi(bd + 3) : 0, false);
        } }
    }
    int count = 0;
    g_hip_touched.store(true);
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count) return LVK_ERR_DEVICE;   // no CPU fallback
    if (hipSetDevice(device) != hipSuccess) return LVK_ERR_DEVICE;
    // LVK_WAIT_POLICY=spin: keep waiting host threads spinning on the completion signal (the runtime's default spins for 100 us,
    // then sleeps until the interrupt).  Process-wide, so opt-in; two A/B pairs of bench runs showed no consistent difference.
    {
        const char* wp = getenv("LVK_WAIT_POLICY");
        if (wp && !strcmp(wp, "spin")) { if (hipSetDeviceFlags(hipDeviceScheduleSpin) != hipSuccess) (void)hipGetLastError(); }
    }
    bind_thread_to_device_node(device);
    lvk_context* c = new (std::nothrow) lvk_context();
    if (!c) return LVK_ERR_DEVICE;
    memset(c, 0, sizeof *c);
    c->device = device; c->own_stream = true;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return LVK_ERR_DEVICE; }
    *out = c;
    return LVK_OK;
}

void lvk_context_destroy(lvk_context* ctx)
{
    if (!ctx) return;
    hipStreamSynchronize(ctx->stream);
    for (int i = 0; i < LVK_SCRATCH_SLOTS; ++i) if (ctx->scratch[i]) hipFree(ctx->scratch[i]);
    if (ctx->own_stream) hipStreamDestroy(ctx->stream);
    delete ctx;
}

lvk_status lvk_context_set_stream(lvk_context* ctx, void* hip_stream)
{
    if (!ctx) return LVK_ERR_ARG;
    // whatever the objects of this context still have queued on the OLD stream (lvk_ekf_process returns with its tail launches
    // outstanding) must not race what the next call queues on the new one: drain it, also when the caller owns it
    if (ctx->stream) LVK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->own_stream) { hipStreamDestroy(ctx->stream); ctx->own_stream = false; }
    if (hip_stream) ctx->stream = (hipStream_t)hip_stream;
    else { LVK_HIP(ctx, hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)); ctx->own_stream = true; }
    return LVK_OK;
}

void* lvk_context_get_stream(const lvk_context* ctx) { return ctx ? (void*)ctx->stream : nullptr; }
lvk_status lvk_sync(lvk_context* ctx) { if (!ctx) return LVK_ERR_ARG; LVK_HIP(ctx, hipStreamSynchronize(ctx->stream)); return LVK_OK; }
const char* lvk_last_error(const lvk_context* ctx) { return ctx ? ctx->err : "null context"; }

lvk_status lvk_malloc(lvk_context* ctx, size_t bytes, void** d_out)
{
    if (!ctx || !d_out) return LVK_ERR_ARG;
    LVK_HIP(ctx, hipMalloc(d_out, bytes ? bytes : 1));
    return LVK_OK;
}
lvk_status lvk_free(lvk_context* ctx, void* d_ptr) { if (!ctx) return LVK_ERR_ARG; LVK_HIP(ctx, hipStreamSynchronize(ctx->stream)); LVK_HIP(ctx, hipFree(d_ptr)); return LVK_OK; }
lvk_status lvk_memcpy_h2d(lvk_context* ctx, void* d_dst, const void* h_src, size_t bytes)
{
    if (!ctx) return LVK_ERR_ARG;
    LVK_HIP(ctx, hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, ctx->stream));
    LVK_HIP(ctx, hipStreamSynchronize(ctx->stream));     // pageable source: finish before the caller reuses it
    return LVK_OK;
}
lvk_status lvk_memcpy_d2h(lvk_context* ctx, void* h_dst, const void* d_src, size_t bytes)
{
    if (!ctx) return LVK_ERR_ARG;
    LVK_HIP(ctx, hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    LVK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LVK_OK;
}
lvk_status lvk_memset(lvk_context* ctx, void* d_dst, int value, size_t bytes)
{
    if (!ctx) return LVK_ERR_ARG;
    LVK_HIP(ctx, hipMemsetAsync(d_dst, value, bytes, ctx->stream));
    return LVK_OK;
}

}  // extern "C"
