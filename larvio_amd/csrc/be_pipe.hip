// be_pipe.hip — the pipelined driver of liblvk_hip.so (lvk_vio_pipe_*; host code only, no kernel): the filter update of frame k on a
// worker thread while the front-end of frame k+1 runs on the caller's.
#include "be_filter.h"
#include <chrono>
#include <deque>

// The reference's driver thread alternates processImage and processFeatures (app/larvioMain.cpp:87-117).  The two halves only
// meet at the feature message and at the shared IMU vector, so here the back-end of frame k runs on its own context (stream)
// in a worker thread while the front-end of frame k+1 runs on the caller's thread.  The one coupling that needs care is the
// IMU vector: processFeatures erases what it consumed and the NEXT processImage integrates gyro samples from whatever is
// left — submit() therefore waits until the erase count of every queued update is known (it is final before any GPU work).
// The count depends on time stamps, on the state time the previous update's IMU batch leaves behind (time stamps again) and on the
// camera-IMU time offset td, which every update moves a little (micro-seconds).  So when the count is the same for td - margin and
// td + margin (LVK_PIPE_TD_MARGIN, 0.5 ms: the bound "image time + td + half an IMU period" is then at least that far from any IMU
// sample) submit() takes it at once from the last published td and the caller's thread runs on while up to two updates are in
// flight; the filter's thread checks the count against the real td when the job starts (never different in any run here; counted in
// lvk_vio_pipe_early_counts if it ever is, and the IMU window is put right for the frames that follow).  Otherwise - an IMU sample
// sample within the margin of the bound - it waits as before.
// Two guards keep a wrong early count from ever reaching the filter (round-3 advice): (1) the IMU view of an update is NOT a copy made at
// submit time but is cut by the filter's thread, when the job starts, from the driver's buffer at the filter's own head (the sum of the TRUE
// counts of the updates before it) - so the filter integrates exactly the samples the sequential loop would, whatever submit() guessed;
// a wrong guess can only have shown a few front-end frames a gyro window that starts one sample off (counted in n_early_wrong, and the
// caller's head is put right at once); (2) submit() only guesses while td is quiet: the largest |td step| of the last eight updates,
// times the updates that can be in flight, must stay well inside the margin - while td is still converging from a bad initial value
// every frame waits for its count.
static double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
struct lvk_vio_pipe {
    lvk_frontend* fe; lvk_ekf* ekf;
    std::vector<lvk_imu> imu; size_t head = 0;          // the driver's imu_msg_buffer = imu[head..) as the CALLER's thread sees it (early counts applied)
    size_t base = 0, fhead = 0;                         // absolute index of imu[0]; absolute index the FILTER has consumed up to (true counts only)
    struct Job { double ts; int slot = -1; std::vector<lvk_imu> view; size_t end_abs = 0; bool precounted = false; double t_submit = 0;      // slot: the front-end's message ring entry; view: cut by the worker from [fhead, end_abs)
                 bool early = false; int n_pre = 0; double t0_pre = 0; };                                                // early: counted by submit() from the published td (to be checked)
    std::vector<float> lat_us;                          // image-in -> state-out of every message-carrying frame (submit entry to update done)
    bool cur_precounted = false;                        // the running job's erase count was already applied by submit()
    std::deque<Job> q;
    std::thread worker; std::mutex mu; std::condition_variable cv_job, cv_state;
    std::atomic<unsigned> gen{0};                       // bumped on every state change: waiters poll it WITHOUT the mutex
    int unknown_consume = 0;                            // queued or running updates whose erase count is not final yet
    // what submit() needs for an early count, all under mu: the filter is initialised, td after the last finished update, the state
    // time after the IMU batch of the last COUNTED job (the filter's own s.t belongs to its thread while a job runs)
    bool steady = false; double td_pub = 0, state_t = 0, td_margin = 5e-4;
    static constexpr int TD_HIST = 32;
    double td_steps[TD_HIST] = {}; long n_td = 0;                       // |td change| of the last TD_HIST finished updates
    double td_factor = 4.0;                             // see td_quiet(); LVK_PIPE_TD_FACTOR (read when the pipeline is created)
    int depth = 2;                                      // updates the caller may have in flight when a frame starts (LVK_PIPE_DEPTH; 1: never more than one update ahead - lower latency, the filter's thread waits for messages)
    long n_early = 0, n_early_wrong = 0;
    int in_flight = 0;                                  // queued + running
    long n_updates = 0, n_msgs = 0;
    lvk_status st = LVK_OK;
    bool stop = false;
    std::vector<lvk_feature_obs> wmsg;                  // the worker's copy of the message it is processing
    lvk_odometry_fn on_update = nullptr; void* on_update_user = nullptr;
    double t_busy = 0, t_idle = 0, t_submit_wait = 0, t_fe = 0;
    struct Ev { double t; int what; };                    // LVK_PIPE_LOG=<file>: event log (0 submit begin, 1 wait done, 2 front-end done,
    std::vector<Ev> log; bool logging = false;            //  3 job queued [4 precounted], 5 job start, 6 job end)
    void ev(int what) { if (logging) log.push_back({now_us(), what}); }   // LVK_EKF_TRACE: where the two threads spend their time (us)
    bool td_quiet() const
    {   // may submit() trust the published td for a count?  (depth + 1) updates can move td before the counted one starts
        // The largest |td step| of the last TD_HIST updates, times td_factor, times the updates in flight, must stay inside the margin.
        // Pipeline fuzz (tools/gpu/fuzz_pipeline.py), 2 of 280 random configurations: a td that is poorly observable (fisheye at 20 Hz
        // publishing; an initial td of milliseconds) sits still for dozens of updates and then steps by 1 ms - 25 times its largest step
        // before - and two counts taken from the stale td were one sample off (the filter's own view never is; two front-end frames
        // integrated their gyro prediction over another window than the sequential loop's).  No history of steps predicts that; what
        // the factor buys is fewer guesses: at 8 (LVK_PIPE_TD_FACTOR=8) those configurations run bit for bit like the sequential loop
        // and bench.py's 20-step line loses 10-15 % of its early counts' benefit (6,700-7,800 against 8,900-9,250 frames/s, same box);
        // at the default 4 the benchmark is where it was and an unconfirmed count is counted and reported (lvk_vio_pipe_early_counts).
        if (n_td < 3) return false;
        double mx = 0; for (int i = 0; i < TD_HIST && i < n_td; ++i) mx = std::max(mx, td_steps[i]);
        return td_factor * (depth + 1) * mx < td_margin;
    }
};

static void pipe_on_consumed(void* user, int n)
{   // fired by the filter once per call, when the number of samples it erases is final (before any GPU work)
    lvk_vio_pipe* p = (lvk_vio_pipe*)user;
    {
        std::lock_guard<std::mutex> lk(p->mu);
        p->fhead += (size_t)n;                          // the filter's own head: true counts only
        if (p->cur_precounted) return;
        p->head += (size_t)n; p->unknown_consume -= 1;
        p->gen.fetch_add(1, std::memory_order_release);
    }
    p->cv_state.notify_all();
}
// Both threads hand over within tens of microseconds: poll briefly before sleeping on the condition variable.
// The poll reads only the generation counter, never the mutex: a waiter that re-locks in a tight loop makes the other thread's
// (short) critical sections queue behind it - that alone added ~30 us to every filter update.
template <typename Pred> static void pipe_wait(lvk_vio_pipe* p, std::unique_lock<std::mutex>& lk, std::condition_variable& cv, Pred pred)
{
    for (int round = 0; round < 64; ++round) {
        if (pred()) return;
        const unsigned seen = p->gen.load(std::memory_order_acquire);
        lk.unlock();
        for (int spin = 0; spin < 4000 && p->gen.load(std::memory_order_acquire) == seen; ++spin) LVK_CPU_RELAX();
        lk.lock();
    }
    cv.wait(lk, pred);
}

static void pipe_worker(lvk_vio_pipe* p)
{
    hipSetDevice(p->ekf->ctx->device);
    if (const char* pin = getenv("LVK_PIN_WORKER")) {       // optional: keep the filter thread on one core (less jitter on big hosts)
        cpu_set_t allowed, one; CPU_ZERO(&allowed); CPU_ZERO(&one);
        if (sched_getaffinity(0, sizeof allowed, &allowed) == 0) {
            int want = atoi(pin), pick = -1, seen = 0;
            for (int c = 0; c < CPU_SETSIZE; ++c) if (CPU_ISSET(c, &allowed)) { if (seen == want) pick = c; ++seen; }
            if (pick < 0) for (int c = CPU_SETSIZE - 1; c >= 0; --c) if (CPU_ISSET(c, &allowed)) { pick = c; break; }
            if (pick >= 0) { CPU_SET(pick, &one); pthread_setaffinity_np(pthread_self(), sizeof one, &one); }
        }
    }
    for (;;) {
        lvk_vio_pipe::Job job;
        const double t0 = now_us();
        {
            std::unique_lock<std::mutex> lk(p->mu);
            pipe_wait(p, lk, p->cv_job, [&] { return p->stop || !p->q.empty(); });
            if (p->q.empty()) return;
            job = std::move(p->q.front()); p->q.pop_front();
            p->cur_precounted = job.precounted;
        }
        const double t1 = now_us();
        {   // this update's IMU view: from the filter's own head to what the driver had pushed when the frame was submitted
            std::lock_guard<std::mutex> lk(p->mu); p->ev(5);
            const size_t lo = std::min(p->fhead - p->base, p->imu.size()), hi = std::min(std::max(job.end_abs - p->base, lo), p->imu.size());
            job.view.assign(p->imu.begin() + (long)lo, p->imu.begin() + (long)hi);
        }
        // The erase count of this update depends on time stamps, the state time and td only - all final now that the previous update
        // is done - so it is published BEFORE this thread blocks on the message: the caller's next frame needs nothing else from here.
        if (!job.precounted && p->ekf->b_first_features && p->ekf->is_gravity_set) {
            double t_after = 0;
            const int n = batch_imu_count(p->ekf, job.ts + p->ekf->td, job.view.data(), (int)job.view.size(), &t_after);
            {
                std::lock_guard<std::mutex> lk(p->mu);
                p->head += (size_t)n; p->unknown_consume -= 1; p->cur_precounted = true; p->state_t = t_after;
                p->gen.fetch_add(1, std::memory_order_release);
            }
            p->cv_state.notify_all();
        } else if (job.early) {
            // counted by submit() from an older td: the same count with the td this update starts from?  (The filter is not affected
            // either way - its view starts at its own head; a wrong guess only moved the window the front-end of the frames submitted
            // since integrated its gyro prediction over.)
            double t_after = 0;
            const int n = batch_imu_count(p->ekf, job.ts + p->ekf->td, job.view.data(), (int)job.view.size(), &t_after);
            if (n != job.n_pre || p->ekf->s.t != job.t0_pre) {
                static const bool verbose = getenv("LVK_VERBOSE") != nullptr;
                if (verbose) fprintf(stderr, "[lvk pipe] early erase count not confirmed at t = %.4f: %d samples counted from td %.6f and state time %.4f, %d with td %.6f and state time %.4f (|td steps| of the last updates up to %.2e)\n",
                                     job.ts, job.n_pre, p->td_pub, job.t0_pre, n, p->ekf->td, p->ekf->s.t, *std::max_element(p->td_steps, p->td_steps + lvk_vio_pipe::TD_HIST));
                std::lock_guard<std::mutex> lk(p->mu);
                const long nh = (long)p->head + (n - job.n_pre);
                p->head = (size_t)std::max(nh, (long)(p->fhead - p->base)); p->head = std::min(p->head, p->imu.size()); p->n_early_wrong += 1;
                if (p->q.empty()) p->state_t = t_after;                 // later jobs were counted from the wrong state time: they are checked in turn
                for (int i = 0; i < lvk_vio_pipe::TD_HIST; ++i) p->td_steps[i] = p->td_margin;   // and nobody guesses again until TD_HIST quiet updates have gone by
                p->gen.fetch_add(1, std::memory_order_release);
            }
        }
        int used = 0, upd = 0;
        // the message itself is collected on THIS thread (the caller's thread queued the frame and went on), and only when the update
        // needs it: IMU integration, covariance propagation and clone augmentation run while the front-end is still tracking
        struct Fetch { lvk_vio_pipe* p; int slot; bool done; } fx{p, job.slot, false};
        auto fetch = [](void* u, const lvk_feature_obs** f, int* n) -> lvk_status {
            Fetch* x = (Fetch*)u;
            lvk_status fs = lvk_frontend_fetch_msg(x->p->fe, x->slot, x->p->wmsg.data(), (int)x->p->wmsg.size(), n);
            *f = x->p->wmsg.data(); x->done = true;
            return fs;
        };
        lvk_status st = p->ekf->process(p->ekf, job.ts, nullptr, 0, job.view.data(), (int)job.view.size(), &used, &upd, fetch, &fx);
        if (!fx.done) { const lvk_feature_obs* f = nullptr; int n = 0; fetch(&fx, &f, &n); }     // a call that returned early still frees its ring entry
        if (st == LVK_OK && upd && p->on_update) { double s30[30]; ekf_quiesce(p->ekf); ekf_state30(p->ekf, s30); p->on_update(p->on_update_user, job.ts, s30); }
        {
            std::lock_guard<std::mutex> lk(p->mu);
            const double t2 = now_us();
            p->t_idle += t1 - t0; p->t_busy += t2 - t1; p->ev(6);
            if (p->lat_us.size() < (size_t)1 << 20) p->lat_us.push_back((float)(t2 - job.t_submit));
            if (st != LVK_OK && p->st == LVK_OK) p->st = st;
            p->n_updates += upd; p->in_flight -= 1;
            const bool was_steady = p->steady;
            p->steady = p->ekf->b_first_features && p->ekf->is_gravity_set;
            if (was_steady && p->steady && upd) { p->td_steps[p->n_td % lvk_vio_pipe::TD_HIST] = fabs(p->ekf->td - p->td_pub); p->n_td += 1; }
            p->td_pub = p->ekf->td;
            p->gen.fetch_add(1, std::memory_order_release);
        }
        p->cv_state.notify_all();
    }
}

extern "C" {

lvk_status lvk_vio_pipe_create(lvk_frontend* fe, lvk_ekf* ekf, lvk_vio_pipe** out)
{
    if (!fe || !ekf || !out) return LVK_ERR_ARG;
    if (lvk_frontend_context(fe) == ekf->ctx)
        return lvk_set_error(ekf->ctx, LVK_ERR_ARG, "lvk_vio_pipe_create: the front-end and the filter must live on different contexts (streams)");
    lvk_vio_pipe* p = new lvk_vio_pipe();
    p->fe = fe; p->ekf = ekf; p->wmsg.resize(8192);
    p->logging = getenv("LVK_PIPE_LOG") != nullptr; if (p->logging) p->log.reserve(1 << 16);
    if (const char* v = getenv("LVK_PIPE_DEPTH")) { const int d = atoi(v); if (d >= 1 && d <= 3) p->depth = d; }
    if (const char* v = getenv("LVK_PIPE_TD_FACTOR")) { const double f = atof(v); if (f >= 1. && f <= 1e6) p->td_factor = f; }      // 3 = the message ring minus the entry being written
    ekf->on_consumed = pipe_on_consumed; ekf->on_consumed_user = p;
    p->worker = std::thread(pipe_worker, p);
    *out = p;
    return LVK_OK;
}

void lvk_vio_pipe_destroy(lvk_vio_pipe* p)
{
    if (!p) return;
    { std::lock_guard<std::mutex> lk(p->mu); p->stop = true; p->gen.fetch_add(1, std::memory_order_release); }
    p->cv_job.notify_all();
    if (p->worker.joinable()) p->worker.join();
    if (p->logging) { if (FILE* f = fopen(getenv("LVK_PIPE_LOG"), "w")) { for (auto& e : p->log) fprintf(f, "%.1f,%d\n", e.t, e.what); fclose(f); } }
    p->ekf->on_consumed = nullptr; p->ekf->on_consumed_user = nullptr;
    delete p;
}

lvk_status lvk_vio_pipe_push_imu(lvk_vio_pipe* p, const lvk_imu* h_imu, int n)
{
    if (!p || (n > 0 && !h_imu)) return LVK_ERR_ARG;
    std::lock_guard<std::mutex> lk(p->mu);
    // compaction: nothing in front of the filter's own head is needed by anybody (queued jobs cut their views from there on, the
    // caller's head is never behind it)
    const size_t done = p->fhead - p->base;
    if (done > 4096 && p->unknown_consume == 0 && done <= p->head) { p->imu.erase(p->imu.begin(), p->imu.begin() + (long)done); p->head -= done; p->base = p->fhead; }
    p->imu.insert(p->imu.end(), h_imu, h_imu + n);
    return LVK_OK;
}

lvk_status lvk_vio_pipe_submit(lvk_vio_pipe* p, const lvk_image* img, double ts, int* has_msg)
{
    if (!p || !has_msg) return LVK_ERR_ARG;
    *has_msg = 0;
    size_t head, end;
    // the image stage (upload, pyramid, ORB planes) does not look at the IMU buffer: queue it before waiting for the erase count
    const double tb = now_us();
    lvk_status st0 = lvk_frontend_begin(p->fe, img, ts);
    if (st0 != LVK_OK) return st0;
    const double t0 = now_us();
    p->t_fe += t0 - tb;
    {
        std::unique_lock<std::mutex> lk(p->mu);
        p->ev(0);
        pipe_wait(p, lk, p->cv_state, [&] { return p->st != LVK_OK || (p->unknown_consume == 0 && p->in_flight <= p->depth); });     // a failed filter never keeps the caller waiting
        if (p->st != LVK_OK) return p->st;
        head = p->head; end = p->imu.size();
        p->ev(1);
    }
    const double t1 = now_us();
    p->t_submit_wait += t1 - t0;
    // only this thread appends to imu, and no update can move `head` until a new job is queued below
    int slot = -1;
    lvk_status st = lvk_frontend_process_async(p->fe, img, ts, p->imu.data() + head, (int)(end - head), has_msg, &slot);
    p->t_fe += now_us() - t1;
    if (p->logging) { std::lock_guard<std::mutex> lk(p->mu); p->ev(2); }
    if (st != LVK_OK || !*has_msg) return st;
    lvk_vio_pipe::Job job;
    job.t_submit = tb;
    job.ts = ts; job.slot = slot;
    {
        std::lock_guard<std::mutex> lk(p->mu);
        job.end_abs = p->base + end;
        const lvk_imu* view = p->imu.data() + head; const int n_view = (int)(end - head);
        // With the worker idle the filter is quiescent: the erase count (timestamps, state time and td only) can be taken here
        // and the next frame need not wait for the worker to wake up.
        lvk_ekf* e = p->ekf;
        bool counted = false;
        if (p->in_flight == 0 && e->b_first_features && e->is_gravity_set) {
            double t_after = 0;
            p->head += (size_t)batch_imu_count(e, ts + e->td, view, n_view, &t_after);
            p->state_t = t_after; p->td_pub = e->td; p->steady = true;
            job.precounted = true; counted = true; p->ev(4);
        } else if (p->in_flight > 0 && p->steady && p->td_quiet()) {
            // every queued job is counted (the wait above), so state_t is the state time this job will start from
            double ta = 0, tb2 = 0;
            const int n_lo = imu_erase_count(p->state_t, ts + p->td_pub - p->td_margin, e->imu_img_time_th, view, n_view, &ta);
            const int n_hi = imu_erase_count(p->state_t, ts + p->td_pub + p->td_margin, e->imu_img_time_th, view, n_view, &tb2);
            if (n_lo == n_hi) {
                job.precounted = true; job.early = true; job.n_pre = n_lo; job.t0_pre = p->state_t;
                p->head += (size_t)n_lo; p->state_t = ta; p->n_early += 1; counted = true; p->ev(7);
            }
        }
        if (!counted) { p->unknown_consume += 1; p->ev(3); }
        p->q.push_back(std::move(job)); p->in_flight += 1; p->n_msgs += 1;
        p->gen.fetch_add(1, std::memory_order_release);
    }
    p->cv_job.notify_one();
    return LVK_OK;
}

lvk_status lvk_vio_pipe_stats(lvk_vio_pipe* p, double* out4, int reset)
{
    if (!p || !out4) return LVK_ERR_ARG;
    std::lock_guard<std::mutex> lk(p->mu);
    out4[0] = p->t_fe; out4[1] = p->t_submit_wait; out4[2] = p->t_busy; out4[3] = p->t_idle;
    if (reset) p->t_busy = p->t_idle = p->t_fe = p->t_submit_wait = 0;
    return LVK_OK;
}

lvk_status lvk_vio_pipe_early_counts(lvk_vio_pipe* p, long* n_early, long* n_wrong)
{
    if (!p) return LVK_ERR_ARG;
    std::lock_guard<std::mutex> lk(p->mu);
    if (n_early) *n_early = p->n_early;
    if (n_wrong) *n_wrong = p->n_early_wrong;
    return LVK_OK;
}

lvk_status lvk_vio_pipe_latency(lvk_vio_pipe* p, float* h_out_us, int cap, int* n_out, int reset)
{
    if (!p || !n_out || (cap > 0 && !h_out_us)) return LVK_ERR_ARG;
    std::lock_guard<std::mutex> lk(p->mu);
    const int n = std::min((int)p->lat_us.size(), cap);
    for (int i = 0; i < n; ++i) h_out_us[i] = p->lat_us[i];
    *n_out = n;
    if (reset) p->lat_us.clear();
    return LVK_OK;
}

lvk_status lvk_vio_pipe_on_update(lvk_vio_pipe* p, lvk_odometry_fn fn, void* user)
{
    if (!p) return LVK_ERR_ARG;
    std::unique_lock<std::mutex> lk(p->mu);
    pipe_wait(p, lk, p->cv_state, [&] { return p->in_flight == 0; });      // the worker reads the pair without the lock
    p->on_update = fn; p->on_update_user = user;
    return LVK_OK;
}

lvk_status lvk_vio_pipe_drain(lvk_vio_pipe* p, long* n_updates, long* n_msgs)
{
    if (!p) return LVK_ERR_ARG;
    std::unique_lock<std::mutex> lk(p->mu);
    pipe_wait(p, lk, p->cv_state, [&] { return p->in_flight == 0; });
    if (n_updates) *n_updates = p->n_updates;
    if (n_msgs) *n_msgs = p->n_msgs;
    return p->st;
}

// one frame through both halves: the front-end waits for its feature message, `process` (lvk_ekf_process, or lvk_ekf_process_async: what
// the adapter classes do under the reference's blocking drivers, processImage returning the message to the caller) takes it
static lvk_status vio_step(lvk_frontend* fe, lvk_ekf* ekf, const lvk_image* img, double ts, const lvk_imu* h_imu, int n_imu, int* n_consumed, int* has_msg, int* updated,
                           lvk_status (*process)(lvk_ekf*, double, const lvk_feature_obs*, int, const lvk_imu*, int, int*, int*))
{
    if (!fe || !ekf || !n_consumed || !has_msg || !updated) return LVK_ERR_ARG;
    *n_consumed = 0; *updated = 0; *has_msg = 0;
    static thread_local std::vector<lvk_feature_obs> msg;
    if (msg.size() < 8192) msg.resize(8192);
    int n_out = 0;
    lvk_status st = lvk_frontend_process(fe, img, ts, h_imu, n_imu, msg.data(), (int)msg.size(), &n_out, has_msg);
    if (st != LVK_OK || !*has_msg) return st;
    return process(ekf, ts, msg.data(), n_out, h_imu, n_imu, n_consumed, updated);
}
lvk_status lvk_vio_process(lvk_frontend* fe, lvk_ekf* ekf, const lvk_image* img, double ts, const lvk_imu* h_imu, int n_imu, int* n_consumed, int* has_msg, int* updated)
{
    return vio_step(fe, ekf, img, ts, h_imu, n_imu, n_consumed, has_msg, updated, lvk_ekf_process);
}
lvk_status lvk_vio_process_deferred(lvk_frontend* fe, lvk_ekf* ekf, const lvk_image* img, double ts, const lvk_imu* h_imu, int n_imu, int* n_consumed, int* has_msg, int* will_update)
{
    return vio_step(fe, ekf, img, ts, h_imu, n_imu, n_consumed, has_msg, will_update, lvk_ekf_process_async);
}

// Localise in the loop (include/lvk_c.h states the steps): the clone's camera pose and covariance from the filter (be_camera_pose.hip),
// the front-end's part (lvk_frontend_localise_obs: match_map's device chain, the gather, one copy back), the batch through
// lvk_ekf_add_landmark_obs.  Host code only; the two handles may live on one context or on two.
lvk_status lvk_vio_localise_map(lvk_frontend* fe, lvk_ekf* ekf, const lvk_align_result* align, int64_t clone_id, double time, double sigma_px,
                                const lvk_map_select_options* select_opt, const lvk_match_options* match_opt, int64_t tag, lvk_localise_info* h_info)
{
    if (!ekf) return LVK_ERR_ARG;
    lvk_ekf* e = ekf;
    if (!fe || !h_info) return lvk_set_error(e->ctx, LVK_ERR_ARG, "lvk_vio_localise_map: bad argument");
    if (clone_id < -1) return lvk_set_error(e->ctx, LVK_ERR_ARG, "lvk_vio_localise_map: clone_id %lld", (long long)clone_id);
    if (clone_id == -1 && !std::isfinite(time)) return lvk_set_error(e->ctx, LVK_ERR_ARG, "lvk_vio_localise_map: time is not finite");
    if (!std::isfinite(sigma_px) || !(sigma_px > 0.)) return lvk_set_error(e->ctx, LVK_ERR_ARG, "lvk_vio_localise_map: sigma_px is not a finite number > 0");
    if (e->on_consumed == pipe_on_consumed) {           // a pipe is attached: only between its drain and the next submit
        lvk_vio_pipe* p = (lvk_vio_pipe*)e->on_consumed_user;
        std::lock_guard<std::mutex> lk(p->mu);
        if (p->in_flight > 0) return lvk_set_error(e->ctx, LVK_ERR_ARG, "lvk_vio_localise_map: the pipe has %d updates in flight (lvk_vio_pipe_drain first)", p->in_flight);
    }
    ekf_quiesce(e);
    if (e->shard.fn) return lvk_set_error(e->ctx, LVK_ERR_UNSUPPORTED, "lvk_vio_localise_map: the sharded update does not apply landmark observations (lvk_ekf_set_shard is set)");
    memset(h_info, 0, sizeof *h_info);
    h_info->status = LVK_LOCALISE_NO_CLONE; h_info->clone_id = -1;
    int i = -1;
    if (e->is_gravity_set) {
        if (clone_id >= 0) i = clone_rank(e, clone_id);
        else for (int k = 0; k < (int)e->clones.size() && i < 0; ++k) if (e->clones[(size_t)k].time == time) i = k;
    }
    if (i < 0) return LVK_OK;
    const Clone& c = e->clones[(size_t)i];
    lvk_camera_pose_job job; memset(&job, 0, sizeof job);
    job.clone_col = e->leg + 6 * i;
    memcpy(job.q_b, c.q, 32); memcpy(job.p_b, c.p, 24); memcpy(job.R_b2c, e->R_b2c, 72); memcpy(job.t_c_b, e->t_c_b, 24);
    lvk_localise_info info; memset(&info, 0, sizeof info);
    info.status = LVK_LOCALISE_QUEUED; info.clone_id = c.id;
    LVK_TRY(lvk_ekf_camera_pose_cov(e->ctx, e->dP[e->cur], e->ld, e->N, &job, info.R_wc, info.p_wc, info.cov_cam));
    e->n_sync++;
    static thread_local std::vector<lvk_landmark_obs> obs;
    static thread_local std::vector<int> idx;
    if (obs.size() < LVK_MAP_MAX_QUERIES) { obs.resize(LVK_MAP_MAX_QUERIES); idx.resize(LVK_MAP_MAX_QUERIES); }
    lvk_map_obs_info oinfo;
    const lvk_status st = lvk_frontend_localise_obs(fe, align, info.R_wc, info.p_wc, info.cov_cam, select_opt, match_opt, sigma_px, obs.data(), idx.data(), &info.map, &oinfo);
    if (st != LVK_OK) {                                 // the front-end's message, on the handle the caller asks for it
        lvk_context* fc = lvk_frontend_context(fe);
        return fc == e->ctx ? st : lvk_set_error(e->ctx, st, "%s", lvk_last_error(fc));
    }
    info.n_ok = oinfo.n_ok; info.n_bad = oinfo.n_bad;
    LVK_TRY(lvk_ekf_add_landmark_obs(e, tag, c.id, c.time, obs.data(), oinfo.n_ok));
    *h_info = info;
    return LVK_OK;
}

}  // extern "C"
