// shard_host_check.cpp - the host paths of avatar_amd/csrc/avt_shard.cpp that need no device, walked by a program of its own so that they
// can run under the host's sanitizers (make -C avatar_amd/csrc shard_host_check_san; no GPU, no Python):
//   - the packed model: pack -> unpack hands avt_model_create a description equal to the original, array for array (with and without the
//     legacy format's fields, and from a copy at another address); every damage case of tests/test_shard_cpu.py
//     test_packed_model_rejects_damage and the other checks of avt_model_unpack; the NULL-array refusal of avt_model_pack
//   - every refusal of include/avt_shard.h that returns before a device is touched, to its text: null handles, null contexts, null
//     out-pointers, the bad arguments of the three creates, world 65 on the shared-memory create, and the device-out-of-range return of 2
// It links avt_shard.cpp alone: what that file calls elsewhere in the library is stubbed below, and a stub that must not be reached aborts.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/avt_shard.h"

struct avt_ctx;
static thread_local std::string g_err;
void avt_set_error(const std::string& s) { g_err = s; }

static int g_failed = 0, g_checked = 0;
#define CHECK(cond) do { ++g_checked; if (!(cond)) { ++g_failed; std::printf("FAILED line %d: %s   [last error: %s]\n", __LINE__, #cond, g_err.c_str()); } } while (0)
static bool refused(int rc, const char* text, int status = 1) { return rc == status && g_err == text; }

// ---- stubs ----------------------------------------------------------------------------------------------------------------------------------
static const avt_model_desc* g_expect = nullptr;      // what avt_model_create must be handed
static int g_created = 0;
static size_t g_len[15];                              // byte length of every array of g_expect

static bool same(const void* a, const void* b, size_t n) { return n == 0 || (a && b && std::memcmp(a, b, n) == 0); }

extern "C" int avt_model_create(const avt_model_desc* d, avt_model** out) {
    const avt_model_desc* e = g_expect;
    if (!e) std::abort();
    bool ok = d->num_points == e->num_points && d->num_joints == e->num_joints && d->num_shape_keys == e->num_shape_keys && d->num_faces == e->num_faces &&
              d->prior_ncomps == e->prior_ncomps && (e->prior_ncomps == 0 || d->prior_ndims == e->prior_ndims) &&
              d->limit_one_joint_per_point == e->limit_one_joint_per_point && !d->joint_shape_reg_base == !e->joint_shape_reg_base && !d->joint_shape_reg == !e->joint_shape_reg;
    const void* got[15] = {d->base_cloud, d->key_clouds, d->parent, d->mesh, d->weights_colptr, d->weights_row, d->weights_val, d->jreg_colptr, d->jreg_row, d->jreg_val,
                           d->prior_weight, d->prior_mean, d->prior_cov, d->joint_shape_reg_base, d->joint_shape_reg};
    const void* want[15] = {e->base_cloud, e->key_clouds, e->parent, e->mesh, e->weights_colptr, e->weights_row, e->weights_val, e->jreg_colptr, e->jreg_row, e->jreg_val,
                            e->prior_weight, e->prior_mean, e->prior_cov, e->joint_shape_reg_base, e->joint_shape_reg};
    for (int i = 0; i < 15; ++i) ok = ok && same(got[i], want[i], g_len[i]) && ((uintptr_t)got[i] % 8 == 0);
    if (!ok) { avt_set_error("stub avt_model_create: the description differs from the packed one"); return 1; }
    ++g_created;
    *out = (avt_model*)&g_created;
    return 0;
}
// reached only with a context, and this program has none
int avt_internal_install_frames(avt_ctx*, int, const int*, const double*, const int*, int) { std::abort(); }
int avt_internal_clear_faults(avt_ctx*) { std::abort(); }
void launch_pack_results(avt_ctx*, int) { std::abort(); }
extern "C" int avt_state_upload(avt_ctx*, int, const double*, const double*, const double*) { std::abort(); }

// ---- a small model --------------------------------------------------------------------------------------------------------------------------
struct Model {
    int V = 6, J = 2, K = 3, F = 2, C = 2, n = 3;
    std::vector<double> base, keys, wval, rval, pw, pm, pc, jsr_base, jsr;
    std::vector<int> parent, mesh, wcol, wrow, rcol, rrow;
    Model() {
        auto fill = [](std::vector<double>& v, size_t n, double a) { v.resize(n); for (size_t i = 0; i < n; ++i) v[i] = a + 0.25 * (double)i; };
        fill(base, 3 * V, 1.0); fill(keys, 3 * V * K, -2.0); fill(pw, C, 0.5); fill(pm, C * n, 0.125); fill(pc, C * n * n, 3.0);
        fill(jsr_base, 3 * J, 7.0); fill(jsr, 3 * J * K, -7.0);
        parent = {-1, 0}; mesh = {0, 1, 2, 3, 4, 5};
        wcol = {0, 1, 2, 4, 5, 6, 7}; wrow = {0, 0, 0, 1, 1, 1, 1}; fill(wval, 7, 0.5);        // V columns
        rcol = {0, 3, 5}; rrow = {0, 1, 2, 4, 5}; fill(rval, 5, 0.2);                            // J columns, rows < V
    }
    avt_model_desc desc(bool legacy) const {
        avt_model_desc d;
        std::memset(&d, 0, sizeof d);
        d.num_points = V; d.num_joints = J; d.num_shape_keys = K; d.num_faces = F;
        d.base_cloud = base.data(); d.key_clouds = keys.data(); d.parent = parent.data(); d.mesh = mesh.data();
        d.weights_colptr = wcol.data(); d.weights_row = wrow.data(); d.weights_val = wval.data();
        d.jreg_colptr = rcol.data(); d.jreg_row = rrow.data(); d.jreg_val = rval.data();
        d.prior_ncomps = C; d.prior_ndims = n; d.prior_weight = pw.data(); d.prior_mean = pm.data(); d.prior_cov = pc.data();
        if (legacy) { d.limit_one_joint_per_point = 1; d.joint_shape_reg_base = jsr_base.data(); d.joint_shape_reg = jsr.data(); }
        return d;
    }
    void lengths(bool legacy) const {
        const size_t l[15] = {(size_t)3 * V * 8, (size_t)3 * V * K * 8, (size_t)J * 4, (size_t)3 * F * 4, (size_t)(V + 1) * 4, 7 * 4, 7 * 8, (size_t)(J + 1) * 4, 5 * 4, 5 * 8,
                              (size_t)C * 8, (size_t)C * n * 8, (size_t)C * n * n * 8, legacy ? (size_t)3 * J * 8 : 0, legacy ? (size_t)3 * J * K * 8 : 0};
        std::memcpy(g_len, l, sizeof l);
    }
};

static std::vector<char> pack(const avt_model_desc& d) {
    size_t n = 0;
    CHECK(avt_model_pack_size(&d, &n) == 0 && n % 8 == 0 && n > 56);
    std::vector<char> b(n);
    CHECK(avt_model_pack(&d, b.data(), n) == 0);
    return b;
}

static void packed_model() {
    Model m;
    avt_model* out = nullptr;
    for (int legacy = 0; legacy < 2; ++legacy) {
        const avt_model_desc d = m.desc(legacy != 0);
        m.lengths(legacy != 0);
        g_expect = &d;
        std::vector<char> b = pack(d);
        const int before = g_created;
        CHECK(avt_model_unpack(b.data(), b.size(), &out) == 0 && g_created == before + 1);
        std::vector<char> far(b.size() + 4096);                      // the block is position independent, and may be longer than its contents
        std::memcpy(far.data() + 1024, b.data(), b.size());
        CHECK(avt_model_unpack(far.data() + 1024, b.size() + 1000, &out) == 0 && g_created == before + 2);
        CHECK(std::memcmp(b.data(), "AVTMODEL", 8) == 0);
    }
    const avt_model_desc d = m.desc(false);
    m.lengths(false);
    g_expect = &d;
    const std::vector<char> b = pack(d);
    const int created = g_created;
    const char* NOT_PACKED = "avt_model_unpack: not a packed model (magic / version / size mismatch)";
    // the damage cases of test_packed_model_rejects_damage: 100 bytes, the last 8 missing, another magic, another version, weights_colptr[V] != nnz
    CHECK(refused(avt_model_unpack(b.data(), 100, &out), NOT_PACKED));
    CHECK(refused(avt_model_unpack(b.data(), b.size() - 8, &out), NOT_PACKED));
    { std::vector<char> x = b; std::memcpy(x.data(), "XXXXXXXX", 8); CHECK(refused(avt_model_unpack(x.data(), x.size(), &out), NOT_PACKED)); }
    { std::vector<char> x = b; x[8] = 7; CHECK(refused(avt_model_unpack(x.data(), x.size(), &out), NOT_PACKED)); }
    const size_t a8 = 7;
    const size_t off_wcol = 56 + 3 * m.V * 8 + 3 * m.V * m.K * 8 + ((m.J * 4 + a8) & ~a8) + ((3 * m.F * 4 + a8) & ~a8);
    const size_t off_rcol = off_wcol + (((m.V + 1) * 4 + a8) & ~a8) + ((7 * 4 + a8) & ~a8) + 7 * 8, off_rrow = off_rcol + (((m.J + 1) * 4 + a8) & ~a8);
    CHECK(std::memcmp(b.data() + off_wcol, m.wcol.data(), (m.V + 1) * 4) == 0 && std::memcmp(b.data() + off_rrow, m.rrow.data(), 5 * 4) == 0);      // (the offsets used below)
    auto with_int = [&](size_t at, int v) { std::vector<char> x = b; std::memcpy(x.data() + at, &v, 4); return x; };
    { auto x = with_int(off_wcol + 4 * m.V, 9); CHECK(refused(avt_model_unpack(x.data(), x.size(), &out), "avt_model_unpack: sparse column pointers do not match the block")); }
    { auto x = with_int(off_wcol, 1); CHECK(refused(avt_model_unpack(x.data(), x.size(), &out), "avt_model_unpack: sparse column pointers do not match the block")); }
    { auto x = with_int(off_rcol + 4 * m.J, 4); CHECK(refused(avt_model_unpack(x.data(), x.size(), &out), "avt_model_unpack: sparse column pointers do not match the block")); }
    { auto x = with_int(off_wcol + 4 * 2, 6); CHECK(refused(avt_model_unpack(x.data(), x.size(), &out), "avt_model_unpack: weight column pointers not monotone")); }
    { auto x = with_int(off_rcol + 4, 6); CHECK(refused(avt_model_unpack(x.data(), x.size(), &out), "avt_model_unpack: regressor column pointers not monotone")); }
    { auto x = with_int(off_rrow + 4, m.V); CHECK(refused(avt_model_unpack(x.data(), x.size(), &out), "avt_model_unpack: regressor row out of range")); }
    { auto x = with_int(off_rrow, -1); CHECK(refused(avt_model_unpack(x.data(), x.size(), &out), "avt_model_unpack: regressor row out of range")); }
    { auto x = with_int(12, 1 << 25); CHECK(refused(avt_model_unpack(x.data(), x.size(), &out), NOT_PACKED)); }      // V beyond what a block may claim
    { auto x = with_int(off_rcol + 4, 1 << 30); CHECK(refused(avt_model_unpack(x.data(), x.size(), &out), "avt_model_unpack: regressor column pointers not monotone")); }   // (no row is walked first)
    { auto x = with_int(44, 4); CHECK(refused(avt_model_unpack(x.data(), x.size(), &out), NOT_PACKED)); }            // a flag nobody defined
    CHECK(refused(avt_model_unpack(nullptr, b.size(), &out), "avt_model_unpack: block too small"));
    CHECK(refused(avt_model_unpack(b.data(), b.size(), nullptr), "avt_model_unpack: block too small"));
    CHECK(refused(avt_model_unpack(b.data(), 55, &out), "avt_model_unpack: block too small"));
    CHECK(g_created == created);
    // avt_model_pack_size / avt_model_pack
    size_t n = 0;
    std::vector<char> buf(b.size());
    CHECK(refused(avt_model_pack_size(nullptr, &n), "avt_model_pack_size: bad model description"));
    CHECK(refused(avt_model_pack_size(&d, nullptr), "avt_model_pack_size: bad model description"));
    CHECK(refused(avt_model_pack(nullptr, buf.data(), buf.size()), "avt_model_pack: bad model description"));
    CHECK(refused(avt_model_pack(&d, nullptr, buf.size()), "avt_model_pack: bad model description"));
    CHECK(refused(avt_model_pack(&d, buf.data(), buf.size() - 1), "avt_model_pack: buffer too small"));
    { avt_model_desc x = d; x.num_points = 0; CHECK(refused(avt_model_pack_size(&x, &n), "avt_model_pack_size: bad model description")); }
    { avt_model_desc x = d; x.weights_colptr = nullptr; CHECK(refused(avt_model_pack_size(&x, &n), "avt_model_pack_size: bad model description")); }
    { avt_model_desc x = d; x.num_joints = AVT_MAX_JOINTS + 1; std::vector<int> col(AVT_MAX_JOINTS + 2, 0); x.jreg_colptr = col.data();
      CHECK(refused(avt_model_pack_size(&x, &n), "avt_model_pack_size: bad model description")); }
    for (int i = 0; i < 10; ++i) {      // every required array in turn (the two column pointers are refused before, with the description)
        avt_model_desc x = d;
        const void** field[10] = {(const void**)&x.base_cloud, (const void**)&x.key_clouds, (const void**)&x.parent, (const void**)&x.mesh, (const void**)&x.weights_row,
                                  (const void**)&x.weights_val, (const void**)&x.jreg_row, (const void**)&x.jreg_val, (const void**)&x.prior_weight, (const void**)&x.prior_cov};
        *field[i] = nullptr;
        CHECK(refused(avt_model_pack(&x, buf.data(), buf.size()), "avt_model_pack: a required array of the model description is NULL"));
    }
    g_expect = nullptr;
}

static void refusals() {
    avt_ctx* c = (avt_ctx*)&g_created;      // never dereferenced: the handle is checked first
    avt_shard* s = nullptr;
    avt_model* m = nullptr;
    avt_stats st[2];
    double d[64] = {0};
    int i[8] = {0};
    const avt_model_desc desc = Model().desc(false);
    // the partition
    CHECK(avt_shard_owner(7, 3) == 1 && avt_shard_owner(7, 0) == 0 && avt_shard_local_count(7, 0, 3) == 3 && avt_shard_local_count(7, 2, 3) == 2);
    CHECK(avt_shard_local_count(3, 5, 8) == 0 && avt_shard_local_count(3, -1, 8) == 0 && avt_shard_local_count(3, 8, 8) == 0 && avt_shard_local_count(3, 0, 0) == 0);
    CHECK(avt_shard_local_index(7, 3) == 2 && avt_shard_local_index(7, 0) == 7 && avt_shard_global_frame(2, 1, 3) == 7);
    // a null handle
    CHECK(avt_shard_rank(nullptr) == -1 && avt_shard_world(nullptr) == 0 && std::strcmp(avt_shard_backend(nullptr), "") == 0);
    avt_shard_destroy(nullptr);
    CHECK(refused(avt_shard_broadcast_model(nullptr, 0, &desc, &m), "avt_shard_broadcast_model: bad argument"));
    CHECK(refused(avt_shard_scatter_frames(nullptr, c, 0, 1, d, i, i, d, d, d), "avt_shard_scatter_frames: bad argument"));
    CHECK(refused(avt_shard_gather_enqueue(nullptr, c, 1), "avt_shard_gather_enqueue: bad argument"));
    CHECK(refused(avt_shard_gather_download(nullptr, c, 1, d, d, d, st), "avt_shard_gather_download: bad argument"));
    CHECK(refused(avt_shard_gather_results(nullptr, c, 1, d, d, d, st), "avt_shard_gather_enqueue: bad argument"));
    CHECK(refused(avt_shard_gather_wait(nullptr), "avt_shard_gather_wait: null argument"));
    CHECK(refused(avt_shard_set_self_exchange(nullptr, 1), "avt_shard_set_self_exchange: null argument"));
    CHECK(refused(avt_shard_barrier(nullptr, c), "avt_shard_barrier: null argument"));
    CHECK(refused(avt_shard_barrier(nullptr, nullptr), "avt_shard_barrier: null argument"));
    // the three creates: bad arguments (checked before anything is opened), then a device this machine does not have
    char id[AVT_SHARD_ID_BYTES];
    std::memset(id, 0x5a, sizeof id);
    typedef int (*create_fn)(int, int, int, const char*, avt_shard**);
    const struct { const char* name; create_fn fn; } creates[3] = {{"avt_shard_create", avt_shard_create}, {"avt_shard_create_loopback", avt_shard_create_loopback},
                                                                    {"avt_shard_create_shm", avt_shard_create_shm}};
    for (const auto& cr : creates) {
        const std::string bad = std::string(cr.name) + ": bad argument", range = std::string(cr.name) + ": device index out of range";
        CHECK(refused(cr.fn(0, 0, 1, nullptr, &s), bad.c_str()));
        CHECK(refused(cr.fn(0, 0, 1, id, nullptr), bad.c_str()));
        CHECK(refused(cr.fn(0, 0, 0, id, &s), bad.c_str()));
        CHECK(refused(cr.fn(0, 0, -2, id, &s), bad.c_str()));
        CHECK(refused(cr.fn(0, -1, 2, id, &s), bad.c_str()));
        CHECK(refused(cr.fn(0, 2, 2, id, &s), bad.c_str()));
        if (cr.fn == avt_shard_create) continue;      // (it opens librccl first, which is no part of this program)
        CHECK(refused(cr.fn(-1, 0, 1, id, &s), range.c_str(), 2));
        CHECK(refused(cr.fn(1 << 20, 0, 1, id, &s), range.c_str(), 2));
    }
    CHECK(refused(avt_shard_create_shm(0, 0, 65, id, &s), "avt_shard_create_shm: bad argument"));
    CHECK(refused(avt_shard_create_shm(0, 64, 65, id, &s), "avt_shard_create_shm: bad argument"));
    CHECK(refused(avt_shard_create_shm(1 << 20, 0, 65, id, &s), "avt_shard_create_shm: bad argument"));      // (before the device is looked at)
    CHECK(s == nullptr);
}

int main() {
    packed_model();
    refusals();
    std::printf("shard_host_check: %d checks, %d failed\n", g_checked, g_failed);
    return g_failed ? 1 : 0;
}
