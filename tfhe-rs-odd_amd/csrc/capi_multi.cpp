// capi_multi.cpp -- multi-device contexts behind include/tfhe_mi355.h (capi_internal.h): key replication (RCCL
// or peer copies), the shard workers, the row split of batched calls and the constructors.
#include <dlfcn.h>
#include <rccl/rccl.h>  // types only: librccl is opened at run time, when keys are replicated

#include "capi_internal.h"

// ---- multi-device contexts ----------------------------------------------------------------------
// SURVEY.md 8b `ctx_create(params, device_mask)` / 8e: ONE process drives several GPUs through one
// context, the way the reference's one process drives its rayon pool (a thread-local ShortintEngine
// per worker, shortint/engine/mod.rs:23-25, and one KS+PBS per block from par_iter,
// integer/server_key/radix_parallel/mul.rs:347-407, through the ShortintBootstrappingKey arms,
// shortint/server_key/mod.rs:104-111,783-857).  A multi-device context owns one single-device context
// ("shard") per listed device; a device may be listed more than once (shards on one GPU then run
// side by side on their own streams).
//   keys: uploaded once, to the first shard, and replicated from its device memory: an RCCL
//     broadcast over xGMI among the distinct devices (librccl opened at run time; ncclCommInitAll
//     over the device list, one rank per distinct device), then device-to-device copies to further
//     shards on the same device.  TFHE_MI355_REPLICATE=copy uses peer copies instead of RCCL,
//     =rccl forces the broadcast even with one distinct device (a one-rank communicator copying
//     into the second shard of that device; a test hook);
//   batched host-pointer calls: split into contiguous shares, one per shard, each run by the shard's
//     own entry point on a thread of its own (its own stream, staging, lock) and joined before the
//     call returns;
//   small calls (the coalesced ones) and submitted requests: round-robin to the shards' coalescers;
//   device-pointer (_async) calls and their scratch queries: the first device's shard (a device
//     pointer belongs to one device; tfhe_mi355_context_device_context hands out each shard).

struct RcclComms {
    void *lib = nullptr;
    decltype(&ncclCommInitAll) init_all = nullptr;
    decltype(&ncclBroadcast) broadcast = nullptr;
    decltype(&ncclGroupStart) group_start = nullptr;
    decltype(&ncclGroupEnd) group_end = nullptr;
    decltype(&ncclCommDestroy) comm_destroy = nullptr;
    decltype(&ncclGetErrorString) error_string = nullptr;
    std::vector<int> devices;  // rank -> device
    std::vector<ncclComm_t> comms;
    ~RcclComms() {
        for (size_t r = 0; r < comms.size(); r++)
            if (comms[r] && comm_destroy) {
                (void)hipSetDevice(devices[r]);
                (void)comm_destroy(comms[r]);
            }
        if (lib) dlclose(lib);
    }
};

namespace {

void check_nccl(const RcclComms &rc, ncclResult_t r, const char *what) {
    if (r != ncclSuccess) fail("%s: %s", what, rc.error_string ? rc.error_string(r) : "RCCL error");
}

// the communicator over `devices` (rank 0 = the source's device), created once per context
RcclComms &rccl_for(TfheMi355Context *m, const std::vector<int> &devices) {
    if (m->rccl && m->rccl->devices == devices) return *m->rccl;
    delete m->rccl;
    m->rccl = nullptr;
    auto rc = std::make_unique<RcclComms>();
    rc->lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!rc->lib) rc->lib = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!rc->lib) fail("RCCL is not available for key replication (%s); TFHE_MI355_REPLICATE=copy uses peer copies",
                       dlerror());
    auto sym = [&](const char *name) {
        void *f = dlsym(rc->lib, name);
        if (!f) fail("librccl lacks %s", name);
        return f;
    };
    rc->init_all = reinterpret_cast<decltype(rc->init_all)>(sym("ncclCommInitAll"));
    rc->broadcast = reinterpret_cast<decltype(rc->broadcast)>(sym("ncclBroadcast"));
    rc->group_start = reinterpret_cast<decltype(rc->group_start)>(sym("ncclGroupStart"));
    rc->group_end = reinterpret_cast<decltype(rc->group_end)>(sym("ncclGroupEnd"));
    rc->comm_destroy = reinterpret_cast<decltype(rc->comm_destroy)>(sym("ncclCommDestroy"));
    rc->error_string = reinterpret_cast<decltype(rc->error_string)>(sym("ncclGetErrorString"));
    rc->devices = devices;
    rc->comms.assign(devices.size(), nullptr);
    check_nccl(*rc, rc->init_all(rc->comms.data(), (int)devices.size(), devices.data()), "ncclCommInitAll");
    m->rccl = rc.release();
    return *m->rccl;
}

// TFHE_MI355_REPLICATE: "auto" (default), "rccl", "copy" ("fail": a replication failure, test hook)
std::string replicate_mode() {
    const char *e = std::getenv("TFHE_MI355_REPLICATE");
    return e && *e ? std::string(e) : std::string("auto");
}

// shard 0's key part -> every other shard (see above); the ready flags are the caller's business
void replicate(TfheMi355Context *m, KeyPart part) {
    auto &S = m->shards;
    TfheMi355Context *src = S[0];
    const size_t bytes = part == KeyPart::Fourier ? src->fourier_bsk_bytes() : src->ksk_len() * sizeof(uint64_t);
    auto buffer = [&](TfheMi355Context *s) -> DeviceBuffer & { return part == KeyPart::Fourier ? s->fbsk : s->ksk; };
    if (!buffer(src).ptr || buffer(src).bytes < bytes) fail("no key on the first device to replicate");
    // distinct devices in order of first appearance (rank 0: the source's) and the shards on each
    std::vector<int> devs;
    std::vector<std::vector<size_t>> on;
    for (size_t i = 0; i < S.size(); i++) {
        const auto it = std::find(devs.begin(), devs.end(), S[i]->device);
        if (it == devs.end()) {
            devs.push_back(S[i]->device);
            on.push_back({i});
        } else {
            on[it - devs.begin()].push_back(i);
        }
    }
    for (size_t i = 1; i < S.size(); i++) {
        check(hipSetDevice(S[i]->device), "hipSetDevice");
        buffer(S[i]).reserve(bytes);
    }
    // the shard of each device that receives the broadcast: the first one on it (on the source's
    // device: a second shard there, else the source itself, in place)
    std::vector<size_t> holder(devs.size());
    for (size_t r = 0; r < devs.size(); r++) holder[r] = r == 0 && on[0].size() > 1 ? on[0][1] : on[r][0];
    const std::string mode = replicate_mode();
    m->replicate_note.clear();
    if (mode == "fail") fail("key replication failed (TFHE_MI355_REPLICATE=fail test hook)");
    bool use_rccl = mode == "rccl" || (mode != "copy" && devs.size() > 1);
    RcclComms *rcp = nullptr;
    if (use_rccl) {
        try {
            rcp = &rccl_for(m, devs);
        } catch (const Failure &e) {
            if (mode == "rccl") throw;
            // auto: librccl missing or its communicator refused -> the peer-copy path
            m->replicate_note = std::string("RCCL unavailable, peer copies: ") + e.what();
            use_rccl = false;
        }
    }
    auto sync_all = [&] {
        for (auto *s : S) {
            check(hipSetDevice(s->device), "hipSetDevice");
            check(hipStreamSynchronize(s->stream), "key replication sync");
        }
    };
    check(hipSetDevice(src->device), "hipSetDevice");
    check(hipStreamSynchronize(src->stream), "key source sync");
    m->replication = use_rccl ? TFHE_MI355_REPLICATION_RCCL
                     : devs.size() > 1 ? TFHE_MI355_REPLICATION_PEER_COPY : TFHE_MI355_REPLICATION_DEVICE_COPY;
    if (use_rccl) {
        RcclComms &rc = *rcp;
        check_nccl(rc, rc.group_start(), "ncclGroupStart");
        for (size_t r = 0; r < devs.size(); r++) {
            check(hipSetDevice(devs[r]), "hipSetDevice");
            TfheMi355Context *h = S[holder[r]];
            const ncclResult_t e =
                rc.broadcast(buffer(src).ptr, buffer(h).ptr, bytes, ncclUint8, 0, rc.comms[r], h->stream);
            if (e != ncclSuccess) {
                (void)rc.group_end();
                check_nccl(rc, e, "ncclBroadcast");
            }
        }
        check_nccl(rc, rc.group_end(), "ncclGroupEnd");
    } else {
        for (size_t r = 0; r < devs.size(); r++) {
            if (holder[r] == 0) continue;
            TfheMi355Context *h = S[holder[r]];
            check(hipSetDevice(h->device), "hipSetDevice");
            check(h->device == src->device
                      ? hipMemcpyAsync(buffer(h).ptr, buffer(src).ptr, bytes, hipMemcpyDeviceToDevice, h->stream)
                      : hipMemcpyPeerAsync(buffer(h).ptr, h->device, buffer(src).ptr, src->device, bytes, h->stream),
                  "key peer copy");
        }
    }
    sync_all();
    for (size_t r = 0; r < devs.size(); r++)  // the other shards of each device: from its holder
        for (size_t i : on[r]) {
            if (i == 0 || i == holder[r]) continue;
            check(hipSetDevice(S[i]->device), "hipSetDevice");
            check(hipMemcpyAsync(buffer(S[i]).ptr, buffer(S[holder[r]]).ptr, bytes, hipMemcpyDeviceToDevice,
                                 S[i]->stream),
                  "key device copy");
        }
    if (part == KeyPart::Ksk)  // each shard repacks its own byte planes for the MFMA keyswitch
        for (size_t i = 1; i < S.size(); i++) {
            check(hipSetDevice(S[i]->device), "hipSetDevice");
            repack_ksk(S[i], S[i]->stream);
        }
    sync_all();
    check(hipSetDevice(src->device), "hipSetDevice");
}

// peer access between every two distinct devices of a multi-device context, so that the peer-copy
// replication (TFHE_MI355_REPLICATE=copy, or auto without RCCL) is a direct xGMI copy rather than
// a staged one; a pair the platform cannot map keeps the staged path (not an error)
void enable_peer_access(const std::vector<int> &devs) {
    std::vector<int> d = devs;
    std::sort(d.begin(), d.end());
    d.erase(std::unique(d.begin(), d.end()), d.end());
    for (int a : d)
        for (int b : d) {
            if (a == b) continue;
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, a, b) != hipSuccess || !can) continue;
            if (hipSetDevice(a) != hipSuccess) continue;
            (void)hipDeviceEnablePeerAccess(b, 0);  // hipErrorPeerAccessAlreadyEnabled is fine too
            (void)hipGetLastError();                 // ... and leaves its code behind
        }
}
}  // namespace

namespace tfhe_mi355::capi {
// the context itself, or the first shard of a multi-device one (device-pointer calls)
TfheMi355Context *primary(TfheMi355Context *c) { return c && c->multi() ? c->shards[0] : c; }

// the shard that takes the next small call / submitted request
TfheMi355Context *pick_shard(TfheMi355Context *m) {
    return m->shards[m->next_shard.fetch_add(1, std::memory_order_relaxed) % m->shards.size()];
}

// key writes of a multi-device context: its own lock (uploads in turn), then every shard's (no
// coalesced batch on any device while the key changes)
std::vector<std::unique_ptr<KeyWrite>> key_write_all(TfheMi355Context *c) {
    std::vector<std::unique_ptr<KeyWrite>> w;
    w.emplace_back(new KeyWrite(c));
    for (auto *s : c->shards) w.emplace_back(new KeyWrite(s));
    return w;
}

void set_ready_all(TfheMi355Context *m, KeyPart part, bool ready) {
    for (auto *s : m->shards) {
        if (part == KeyPart::Fourier) s->fbsk_ready = ready;
        else s->ksk_ready = ready;
    }
}

// a batched host-pointer call of a multi-device context: shard i runs rows [count i / S, count (i+1)
// / S) through `f(shard, first, count)` (an entry point of the shard, 0 = ok), shard 0 on the calling
// thread and the others on threads of their own; joined, then the first failure is reported
// The whole call holds the multi-device context's key lock shared, so a concurrent key upload
// (key_write_all: this context exclusively first) lands before or after it, never between two
// shards' shares.
void split_rows(TfheMi355Context *m, size_t count, const std::function<int(TfheMi355Context *, size_t, size_t)> &f) {
    const size_t S = m->shards.size();
    KeyRead keys(m);
    std::vector<std::string> errs(S);
    auto run = [&](size_t i) {
        const size_t a = count * i / S, b = count * (i + 1) / S;
        if (a == b) return;
        try {
            if (f(m->shards[i], a, b - a) != TFHE_MI355_OK) errs[i] = tfhe_mi355_last_error();
        } catch (const std::exception &e) {
            errs[i] = e.what();
        }
    };
    std::mutex dm;
    std::condition_variable dcv;
    size_t left = 0;
    for (size_t i = 1; i < S; i++) {
        if (count * i / S == count * (i + 1) / S) continue;
        left++;
        m->workers[i - 1]->post([&, i] {
            run(i);
            std::lock_guard<std::mutex> g(dm);
            if (--left == 0) dcv.notify_one();
        });
    }
    run(0);
    {
        std::unique_lock<std::mutex> g(dm);
        dcv.wait(g, [&] { return left == 0; });
    }
    for (size_t i = 0; i < S; i++)
        if (!errs[i].empty()) fail("device %d (shard %zu): %s", m->shards[i]->device, i, errs[i].c_str());
}

// a key upload of a multi-device context: `first` (the same entry point) on the first device's
// shard, then the key part replicated to the other shards (RCCL broadcast / device copies)
void multi_key_upload(TfheMi355Context *m, KeyPart part, const std::function<int(TfheMi355Context *)> &first) {
    auto w = key_write_all(m);
    set_ready_all(m, part, false);
    try {
        abi(first(m->shards[0]));
        replicate(m, part);
    } catch (...) {  // the first shard may hold the new key already: no shard serves a half-replicated one
        set_ready_all(m, part, false);
        throw;
    }
    set_ready_all(m, part, true);
}

// tfhe_mi355_context_destroy of a multi-device context: every shard (each reports its own queued requests),
// then the communicator
void destroy_multi(TfheMi355Context *ctx) {
    ctx->workers.clear();  // joins the shard workers (a split call still running finishes first)
    std::string errs;
    for (auto *s : ctx->shards) {
        s->owner = nullptr;
        if (tfhe_mi355_context_destroy(s) != TFHE_MI355_OK)
            errs += std::string(errs.empty() ? "" : "; ") + tfhe_mi355_last_error();
    }
    delete ctx->rccl;
    delete ctx;
    if (!errs.empty()) fail("%s", errs.c_str());
}
}  // namespace tfhe_mi355::capi

extern "C" {

int tfhe_mi355_context_create_devices(const TfheMi355Parameters *params, const int *devices, size_t device_count,
                                      TfheMi355Context **out_ctx) {
    return guarded([&] {
        if (!out_ctx) fail("null out_ctx");
        *out_ctx = nullptr;
        if (!params || (!devices && device_count)) fail("null argument");
        validate_parameters(*params);
        int visible = 0;
        check(hipGetDeviceCount(&visible), "hipGetDeviceCount");
        std::vector<int> devs(devices, devices + device_count);
        if (devs.empty())  // no list: every visible device
            for (int d = 0; d < visible; d++) devs.push_back(d);
        if (devs.empty()) fail("no GPU visible");
        if (devs.size() > 64) fail("at most 64 devices per context (%zu listed)", devs.size());
        for (int d : devs)
            if (d < 0 || d >= visible) fail("device %d is not visible (%d devices)", d, visible);
        if (devs.size() == 1) {
            *out_ctx = create_single(*params, devs[0]);
            return;
        }
        auto *m = new TfheMi355Context();
        m->p = *params;
        m->device = devs[0];
        try {
            for (int d : devs) {
                m->shards.push_back(create_single(*params, d));
                m->shards.back()->owner = m;
            }
            for (size_t i = 1; i < devs.size(); i++) {
                m->workers.emplace_back(new ShardWorker());
                ShardWorker *w = m->workers.back().get();
                w->t = std::thread([w] { w->loop(); });
            }
            enable_peer_access(devs);
        } catch (...) {
            tfhe_mi355_context_destroy(m);
            throw;
        }
        *out_ctx = m;
    });
}

int tfhe_mi355_context_devices(TfheMi355Context *ctx, size_t *count) {
    return guarded([&] {
        if (!ctx || !count) fail("null argument");
        *count = ctx->multi() ? ctx->shards.size() : 1;
    });
}

int tfhe_mi355_context_replication(TfheMi355Context *ctx, int *mode, const char **note) {
    return guarded([&] {
        if (!ctx || !mode) fail("null argument");
        *mode = ctx->multi() ? ctx->replication : TFHE_MI355_REPLICATION_NONE;
        if (note) *note = ctx->replicate_note.c_str();
    });
}

int tfhe_mi355_context_device_context(TfheMi355Context *ctx, size_t index, TfheMi355Context **out_ctx,
                                      int *device) {
    return guarded([&] {
        if (!out_ctx) fail("null out_ctx");
        *out_ctx = nullptr;
        if (!ctx) fail("null ctx");
        const size_t n = ctx->multi() ? ctx->shards.size() : 1;
        if (index >= n) fail("device index %zu out of range (%zu devices)", index, n);
        TfheMi355Context *s = ctx->multi() ? ctx->shards[index] : ctx;
        if (device) *device = s->device;
        *out_ctx = s;
    });
}

}  // extern "C"
