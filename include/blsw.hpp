// C++ host side above the C ABI of blsw.h, with the names of the reference's gadget interface (src/constraints.rs, src/bls.rs) so that a
// caller — and the parity tests — read like the reference's own tests (constraints.rs:318-376). Header only, C++17, HIP runtime API for the
// device buffers; no torch. The reference is a Rust crate: its maintainers bind blsw.h directly; this header is the same
// boundary for a C++ host, and the statement-by-statement mirror of what the Rust side does around `verify`.
//
// One difference in shape, stated once: the reference builds ONE ConstraintSystemRef per (pk, msg, sig) instance and synthesises it on a CPU
// thread; here a ConstraintSystem stands for n independent systems of one shape, generated together on the GPU. Everything else keeps its name:
//   PublicKey::try_from / Signature::try_from          bls.rs:219-242, 316-339 (compressed ZCash encoding; decoded on the device)
//   UInt8::new_witness_vec / new_input_vec              constraints.rs:341
//   ParametersVar / PublicKeyVar / SignatureVar::new_variable(cs, value, AllocationMode)   constraints.rs:194-249
//   BlsSignatureVerifyGadget::verify(&params, &pk, &msg, &sig) -> Boolean                  constraints.rs:90-128
//   BlsSignatureVerifyGadget::aggregate_verify(&params, &keys, &bitmap, &msg, &sig) -> (Boolean, UInt32)   constraints.rs:153-191
//   cs.num_constraints(), cs.num_witness_variables(), Boolean::value()                     constraints.rs:369-373
//   BLS::sign / BLS::verify (the native scheme, batched)                                   bls.rs:411-458
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <random>
#include <vector>

#include "blsw.h"

namespace blsw {

class Error : public std::runtime_error {
   public:
    int code;
    Error(const std::string& what, int c) : std::runtime_error(what + " failed: " + std::to_string(c)), code(c) {}
};
inline void check(int rc, const char* what) {
    if (rc != BLSW_OK) throw Error(what, rc);
}
inline void hip_check(hipError_t e, const char* what) {
    if (e != hipSuccess) throw Error(std::string(what) + " (" + hipGetErrorString(e) + ")", BLSW_ERR_HIP);
}

namespace detail {
class DeviceBytes {  // RAII device allocation
   public:
    DeviceBytes() = default;
    explicit DeviceBytes(size_t bytes) : n_(bytes) { hip_check(hipMalloc(&p_, bytes ? bytes : 1), "hipMalloc"); }
    DeviceBytes(const DeviceBytes&) = delete;
    DeviceBytes& operator=(const DeviceBytes&) = delete;
    DeviceBytes(DeviceBytes&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; }
    DeviceBytes& operator=(DeviceBytes&& o) noexcept {
        if (this != &o) {
            if (p_) (void)hipFree(p_);
            p_ = o.p_;
            n_ = o.n_;
            o.p_ = nullptr;
        }
        return *this;
    }
    ~DeviceBytes() {
        if (p_) (void)hipFree(p_);
    }
    void* get() const { return p_; }
    size_t size() const { return n_; }
    void upload(const void* src, size_t bytes) { hip_check(hipMemcpy(p_, src, bytes, hipMemcpyHostToDevice), "hipMemcpy H2D"); }
    void download(void* dst, size_t bytes, size_t offset = 0) const {
        hip_check(hipMemcpy(dst, static_cast<const char*>(p_) + offset, bytes, hipMemcpyDeviceToHost), "hipMemcpy D2H");
    }

   private:
    void* p_ = nullptr;
    size_t n_ = 0;
};
inline std::vector<uint8_t> unhex(std::string s, size_t want) {
    if (s.rfind("0x", 0) == 0) s = s.substr(2);
    if (s.size() != 2 * want) throw Error("hex string of " + std::to_string(want) + " bytes", BLSW_ERR_ARG);
    std::vector<uint8_t> out(want);
    for (size_t i = 0; i < want; i++) {
        auto nib = [&](char c) -> int {
            if (c >= '0' && c <= '9') return c - '0';
            if (c >= 'a' && c <= 'f') return c - 'a' + 10;
            if (c >= 'A' && c <= 'F') return c - 'A' + 10;
            throw Error("hex digit", BLSW_ERR_ARG);
        };
        out[i] = (uint8_t)(nib(s[2 * i]) * 16 + nib(s[2 * i + 1]));
    }
    return out;
}
}  // namespace detail

// A key set shared by many aggregate_verify instances (blsw_keyset_t, ABI 15): the committee's K keys are allocated as witnesses ONCE, and every step of
// an engine created with options.shared_keys = 1 that names the set gets the allocation witnesses copied into the head of its vectors. Owns the handle
// and its device buffer; must outlive every step submitted with it. d_pks_xy: [K][12] u64 affine Montgomery on the device, (0, 0) = infinity (what
// blsw_decode_batch writes). The submit / expand members are the engine's keyset entry points with this set as their `ks`.
class KeySet {
   public:
    KeySet(const uint64_t* d_pks_xy, uint32_t n_keys, uint32_t output_form = 0, int device = -1, void* stream = nullptr) : n_keys_(n_keys) {
        uint64_t bytes = 0;
        check(blsw_keyset_bytes(n_keys, &bytes), "blsw_keyset_bytes");
        if (device >= 0) hip_check(hipSetDevice(device), "hipSetDevice");
        buffer_ = detail::DeviceBytes(bytes);  // hipMalloc: 256-byte aligned
        check(blsw_keyset_create(&ks_, d_pks_xy, n_keys, output_form, device, buffer_.get(), bytes, stream), "blsw_keyset_create");
    }
    KeySet(const KeySet&) = delete;
    KeySet& operator=(const KeySet&) = delete;
    KeySet(KeySet&& o) noexcept : ks_(o.ks_), n_keys_(o.n_keys_), buffer_(std::move(o.buffer_)) { o.ks_ = nullptr; }
    ~KeySet() {
        if (ks_) (void)blsw_keyset_destroy(ks_);
    }
    const blsw_keyset_t* get() const { return ks_; }
    uint32_t n_keys() const { return n_keys_; }
    // the table [n_keys * 1942][6] u64 on the device, in the set's output form
    const uint64_t* table(uint64_t* n_elements = nullptr) const {
        const uint64_t* t = nullptr;
        uint64_t n = 0;
        check(blsw_keyset_table(ks_, &t, &n), "blsw_keyset_table");
        if (n_elements) *n_elements = n;
        return t;
    }
    void submit_aggregate(blsw_engine_t* e, const uint8_t* d_bitmap, const uint64_t* d_sig_xy, const uint8_t* d_msg, uint64_t* d_instance, uint64_t* d_witness,
                          uint64_t witness_stride, int32_t* d_result, uint32_t* d_count, void* stream = nullptr) const {
        check(blsw_engine_submit_aggregate_keyset(e, ks_, d_bitmap, d_sig_xy, d_msg, d_instance, d_witness, witness_stride, d_result, d_count, stream),
              "blsw_engine_submit_aggregate_keyset");
    }
    void submit_aggregate_compact(blsw_engine_t* e, const uint8_t* d_bitmap, const uint64_t* d_sig_xy, const uint8_t* d_msg, void* d_compact, int32_t* d_result,
                                  uint32_t* d_count, void* stream = nullptr) const {
        check(blsw_engine_submit_aggregate_keyset_compact(e, ks_, d_bitmap, d_sig_xy, d_msg, d_compact, d_result, d_count, stream),
              "blsw_engine_submit_aggregate_keyset_compact");
    }
    void expand_compact(blsw_engine_t* e, const void* d_compact, uint64_t* d_witness, uint64_t witness_stride, void* stream = nullptr) const {
        check(blsw_engine_expand_compact_keyset(e, ks_, d_compact, d_witness, witness_stride, stream), "blsw_engine_expand_compact_keyset");
    }

   private:
    blsw_keyset_t* ks_ = nullptr;
    uint32_t n_keys_ = 0;
    detail::DeviceBytes buffer_;
};

// ark_r1cs_std::alloc::AllocationMode. PublicKeyVar / SignatureVar: Witness (the reference's circuits) or Input (the point's coordinates become
// instance_assignment[1..]); ParametersVar: Constant or Witness.
enum class AllocationMode { Constant, Input, Witness };

// bls.rs:23-38: Parameters::default() is the standard G1 generator — the only value the engine knows
struct Parameters {};
// bls.rs:219-242 / 316-339: the compressed encodings. try_from checks the text form here; flags, x < p, curve and subgroup membership are
// checked by the device decode when the variable is used, with the outcome in ConstraintSystem::status() (the reference's test harness
// replaces a point that does not decode by the default and expects `false`: tests/tests.rs:244-263 — that rule is applied by verify)
struct PublicKey {
    std::array<uint8_t, 48> bytes;
    static PublicKey try_from(const std::string& hex) {
        PublicKey k;
        auto b = detail::unhex(hex, 48);
        std::memcpy(k.bytes.data(), b.data(), 48);
        return k;
    }
};
struct Signature {
    std::array<uint8_t, 96> bytes;
    static Signature try_from(const std::string& hex) {
        Signature s;
        auto b = detail::unhex(hex, 96);
        std::memcpy(s.bytes.data(), b.data(), 96);
        return s;
    }
};

// A resident registry of public keys (blsw_registry_t): room for `capacity` keys (1 .. 2^24), decoded ONCE when they are appended — with the
// subgroup check, asynchronously on the stream given — and summed through index lists by BLS::fast_aggregate_verify_indexed. Owns the handle and
// its device buffer. A verify call must be ordered behind the appends it relies on; the object is not thread-safe.
class KeyRegistry {
   public:
    explicit KeyRegistry(uint32_t capacity, int device = -1) : capacity_(capacity), device_(device) {
        uint64_t bytes = 0;
        check(blsw_registry_bytes(capacity, &bytes), "blsw_registry_bytes");
        if (device_ < 0) hip_check(hipGetDevice(&device_), "hipGetDevice");
        const OnDevice on(device_);
        buffer_ = detail::DeviceBytes(bytes);  // hipMalloc: 256-byte aligned
        check(blsw_registry_create(&r_, capacity, device_, buffer_.get(), bytes), "blsw_registry_create");
    }
    KeyRegistry(const KeyRegistry&) = delete;
    KeyRegistry& operator=(const KeyRegistry&) = delete;
    KeyRegistry(KeyRegistry&& o) noexcept : r_(o.r_), capacity_(o.capacity_), device_(o.device_), buffer_(std::move(o.buffer_)) { o.r_ = nullptr; }
    ~KeyRegistry() {
        if (r_) (void)blsw_registry_destroy(r_);
    }
    const blsw_registry_t* get() const { return r_; }
    uint32_t capacity() const { return capacity_; }
    uint32_t size() const {
        uint32_t n = 0;
        check(blsw_registry_size(r_, &n), "blsw_registry_size");
        return n;
    }
    // d_pks48 [count][48] compressed keys on the device become keys [size, size + count)
    void append_device(const uint8_t* d_pks48, uint32_t count, void* stream = nullptr) { check(blsw_registry_append(r_, d_pks48, count, stream), "blsw_registry_append"); }
    // host keys: uploaded, appended on the NULL stream, and waited for (the staging copy is released on return)
    void append(const std::vector<PublicKey>& keys) {
        if (keys.empty()) return;
        std::vector<uint8_t> pk(keys.size() * 48);
        for (size_t k = 0; k < keys.size(); k++) std::memcpy(&pk[48 * k], keys[k].bytes.data(), 48);
        const OnDevice on(device_);
        detail::DeviceBytes d(pk.size());
        d.upload(pk.data(), pk.size());
        append_device(static_cast<const uint8_t*>(d.get()), (uint32_t)keys.size());
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
    }
    // the keys' BLSW_ST_* [size], downloaded (waits for the device)
    std::vector<int32_t> key_status() const {
        const int32_t* d = nullptr;
        check(blsw_registry_key_status(r_, &d), "blsw_registry_key_status");
        std::vector<int32_t> st(size());
        const OnDevice on(device_);
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        if (!st.empty()) hip_check(hipMemcpy(st.data(), d, st.size() * 4, hipMemcpyDeviceToHost), "hipMemcpy");
        return st;
    }

    // sum_p s_p * key[index_p] per list, by the bucket method (blsw_registry_msm_batch): one list of indices and one of scalars (32 little-endian
    // bytes below r, PUBLIC) per entry of the outer vectors. status (optional) [n] as the header states it; a failing list gives an all-zero key.
    std::vector<PublicKey> msm(const std::vector<std::vector<uint32_t>>& indices, const std::vector<std::vector<std::array<uint8_t, 32>>>& scalars,
                               std::vector<int32_t>* status = nullptr, uint32_t window_bits = 0) const {
        const size_t n = indices.size();
        if (n == 0 || scalars.size() != n) throw Error("KeyRegistry::msm: one list of scalars per list of indices, at least one list", BLSW_ERR_ARG);
        std::vector<uint64_t> offsets(n + 1, 0);
        std::vector<uint32_t> flat;
        std::vector<uint8_t> rows;
        for (size_t i = 0; i < n; i++) {
            if (scalars[i].size() != indices[i].size()) throw Error("KeyRegistry::msm: one scalar per index", BLSW_ERR_ARG);
            flat.insert(flat.end(), indices[i].begin(), indices[i].end());
            for (const auto& sc : scalars[i]) rows.insert(rows.end(), sc.begin(), sc.end());
            offsets[i + 1] = flat.size();
        }
        uint64_t bytes = 0;
        check(blsw_registry_msm_workspace_bytes(n, flat.size(), window_bits, &bytes), "blsw_registry_msm_workspace_bytes");
        const OnDevice on(device_);
        detail::DeviceBytes d_idx(flat.size() * 4 + 4), d_off(offsets.size() * 8), d_sc(rows.size() + 32), d_out(n * 48), d_st(n * 4), ws(bytes + 256);
        if (!flat.empty()) d_idx.upload(flat.data(), flat.size() * 4);
        if (!rows.empty()) d_sc.upload(rows.data(), rows.size());
        d_off.upload(offsets.data(), offsets.size() * 8);
        check(blsw_registry_msm_batch(r_, flat.empty() ? nullptr : static_cast<const uint32_t*>(d_idx.get()), flat.size(), static_cast<const uint64_t*>(d_off.get()),
                                      flat.empty() ? nullptr : static_cast<const uint8_t*>(d_sc.get()), n, window_bits, static_cast<uint8_t*>(d_out.get()),
                                      static_cast<int32_t*>(d_st.get()), ws.get(), bytes + 256, nullptr),
              "blsw_registry_msm_batch");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        std::vector<uint8_t> o(n * 48);
        d_out.download(o.data(), o.size());
        if (status) {
            status->resize(n);
            d_st.download(status->data(), n * 4);
        }
        std::vector<PublicKey> out(n);
        for (size_t i = 0; i < n; i++) std::memcpy(out[i].bytes.data(), &o[48 * i], 48);
        return out;
    }

    int device() const { return device_; }

   private:
    // the registry's device made current for a scope; the caller's current device is as it was afterwards, also when the scope throws
    struct OnDevice {
        int prev = -1;
        explicit OnDevice(int device) {
            int cur = -1;
            hip_check(hipGetDevice(&cur), "hipGetDevice");
            if (cur == device) return;
            hip_check(hipSetDevice(device), "hipSetDevice");
            prev = cur;
        }
        OnDevice(const OnDevice&) = delete;
        OnDevice& operator=(const OnDevice&) = delete;
        ~OnDevice() {
            if (prev >= 0) (void)hipSetDevice(prev);
        }
    };
    blsw_registry_t* r_ = nullptr;
    uint32_t capacity_ = 0;
    int device_ = -1;
    detail::DeviceBytes buffer_;
};

// n independent constraint systems of one circuit shape (constraints.rs:335: `ConstraintSystem::<Fq>::new_ref()`, once per instance there)
class ConstraintSystem {
   public:
    ConstraintSystem(size_t n, uint32_t msg_len, int device = -1) : n_(n), msg_len_(msg_len), device_(device) {
        if (n == 0) throw Error("ConstraintSystem(n = 0)", BLSW_ERR_ARG);
        check(blsw_layout(msg_len, &layout_), "blsw_layout");
    }
    ~ConstraintSystem() {
        if (r1cs_) blsw_r1cs_destroy(r1cs_);
        if (engine_) blsw_engine_destroy(engine_);
    }
    ConstraintSystem(const ConstraintSystem&) = delete;
    ConstraintSystem& operator=(const ConstraintSystem&) = delete;

    size_t num_instances() const { return n_; }
    uint32_t msg_len() const { return msg_len_; }
    // cs.num_witness_variables() / num_instance_variables() of every one of the n systems (shape properties; after ParametersVar::new_variable
    // they describe the circuit with that parameter mode)
    uint64_t num_witness_variables() const { return layout_.n_witness; }
    uint64_t num_instance_variables() const { return layout_.n_instance_vars; }
    // cs.num_constraints(): the library synthesises the system symbolically on the host (a few seconds, once per call)
    uint64_t num_constraints() const { return matrices_info().n_constraints; }
    // cs.which_is_unsatisfied() of every one of the n systems after verify, on the device (blsw_r1cs_check over the witness and instance vectors
    // this object holds): the index of the first unsatisfied constraint, or -1. The first call synthesises the matrices on the host and encodes
    // them on the device (a few seconds, once per object).
    std::vector<int64_t> which_is_unsatisfied() {
        if (!witness_.get()) throw Error("which_is_unsatisfied before verify", BLSW_ERR_ARG);
        if (!r1cs_) build_checker();
        detail::DeviceBytes d_bad(n_ * 8);
        const bool io = layout_.n_instance_vars > 1;
        check(blsw_r1cs_check(r1cs_, io ? static_cast<const uint64_t*>(instance_.get()) : nullptr, layout_.n_instance_vars, static_cast<const uint64_t*>(witness_.get()),
                              layout_.n_witness, n_, 0, static_cast<int64_t*>(d_bad.get()), nullptr, nullptr),
              "blsw_r1cs_check");
        std::vector<int64_t> bad(n_);
        d_bad.download(bad.data(), n_ * 8);
        return bad;
    }
    // The same for a step of this circuit shape in compact wire form (blsw_r1cs_check_compact): d_compact is a device buffer of layout.total bytes —
    // a step another rank's engine produced with blsw_engine_submit_compact — and layout its blsw_compact_layout; layout.n verdicts. The step is
    // read where it lies: no blsw_engine_expand_compact, no witness vectors. A circuit with public inputs takes d_instance [layout.n][n_instance_vars][6]
    // (device; the compact form carries witnesses only), by default the instance vectors this object's verify wrote (then layout.n == n).
    std::vector<int64_t> which_is_unsatisfied(const blsw_compact_layout_t& layout, const void* d_compact, const uint64_t* d_instance = nullptr) {
        if (!r1cs_) build_checker();
        if (layout_.n_instance_vars > 1 && !d_instance) {
            if (!instance_.get() || layout.n != n_) throw Error("which_is_unsatisfied(compact): instance vectors of layout.n systems", BLSW_ERR_ARG);
            d_instance = static_cast<const uint64_t*>(instance_.get());
        }
        detail::DeviceBytes d_bad(layout.n * 8);
        check(blsw_r1cs_check_compact(r1cs_, &layout, d_compact, d_instance, d_instance ? layout_.n_instance_vars : 0, static_cast<int64_t*>(d_bad.get()), nullptr, nullptr),
              "blsw_r1cs_check_compact");
        std::vector<int64_t> bad(layout.n);
        d_bad.download(bad.data(), layout.n * 8);
        return bad;
    }
    // The same for a step of a shared-keys engine (blsw_r1cs_check_compact_keyset): its buffer carries no key rows, `layout` is blsw_compact_layout_keyset's
    // and the head of every vector is the receiver's own KeySet (Montgomery form). skip_head_rows: only the rows behind the ones that read the head
    // alone — check(keys) vouches for those, once per set instead of once per instance. Reported rows keep their numbers either way.
    std::vector<int64_t> which_is_unsatisfied(const blsw_compact_layout_t& layout, const void* d_compact, const KeySet& keys, bool skip_head_rows,
                                              const uint64_t* d_instance = nullptr) {
        if (!r1cs_) build_checker();
        if (layout_.n_instance_vars > 1 && !d_instance) {
            if (!instance_.get() || layout.n != n_) throw Error("which_is_unsatisfied(compact, keys): instance vectors of layout.n systems", BLSW_ERR_ARG);
            d_instance = static_cast<const uint64_t*>(instance_.get());
        }
        detail::DeviceBytes d_bad(layout.n * 8);
        check(blsw_r1cs_check_compact_keyset(r1cs_, &layout, d_compact, keys.get(), skip_head_rows ? BLSW_R1CS_HEAD_SKIP : BLSW_R1CS_HEAD_CHECK, d_instance,
                                             d_instance ? layout_.n_instance_vars : 0, static_cast<int64_t*>(d_bad.get()), nullptr, nullptr),
              "blsw_r1cs_check_compact_keyset");
        std::vector<int64_t> bad(layout.n);
        d_bad.download(bad.data(), layout.n * 8);
        return bad;
    }
    // The same for a step of the N+1-pair product (blsw_r1cs_check_compact_multi): `layout` is blsw_compact_layout_multi's, of the engine that produced
    // the step with blsw_engine_submit_multi_compact. Every pair family of the system is evaluated with one pair per lane, the other rows with one
    // instance per lane; the first call per layout finds the families (pair_families below).
    std::vector<int64_t> which_is_unsatisfied(const blsw_compact_layout_multi_t& layout, const void* d_compact, const uint64_t* d_instance = nullptr) {
        if (!r1cs_) build_checker();
        if (layout_.n_instance_vars > 1 && !d_instance) {
            if (!instance_.get() || layout.n != n_) throw Error("which_is_unsatisfied(compact multi): instance vectors of layout.n systems", BLSW_ERR_ARG);
            d_instance = static_cast<const uint64_t*>(instance_.get());
        }
        detail::DeviceBytes d_bad(layout.n * 8);
        check(blsw_r1cs_check_compact_multi(r1cs_, &layout, d_compact, d_instance, d_instance ? layout_.n_instance_vars : 0, static_cast<int64_t*>(d_bad.get()), nullptr,
                                            nullptr),
              "blsw_r1cs_check_compact_multi");
        std::vector<int64_t> bad(layout.n);
        d_bad.download(bad.data(), layout.n * 8);
        return bad;
    }
    // {first row, rows per pair} of every pair family of this system under `layout` (blsw_r1cs_handle_pair_families)
    std::vector<std::pair<uint64_t, uint64_t>> pair_families(const blsw_compact_layout_multi_t& layout) {
        if (!r1cs_) build_checker();
        uint64_t count = 0;
        check(blsw_r1cs_handle_pair_families(r1cs_, &layout, 0, nullptr, nullptr, &count), "blsw_r1cs_handle_pair_families");
        std::vector<uint64_t> first(count), rows(count);
        check(blsw_r1cs_handle_pair_families(r1cs_, &layout, count, first.data(), rows.data(), &count), "blsw_r1cs_handle_pair_families");
        std::vector<std::pair<uint64_t, uint64_t>> out;
        for (uint64_t f = 0; f < count; f++) out.emplace_back(first[f], rows[f]);
        return out;
    }
    // The committee, once (blsw_r1cs_check_keyset): the first unsatisfied one of the rows that read nothing but the set's table, or -1; *first_unreduced
    // (optional): the index of z of the first table element >= p, or -1. The table in either element form.
    int64_t check(const KeySet& keys, int64_t* first_unreduced = nullptr) {
        if (!r1cs_) build_checker();
        detail::DeviceBytes d_out(16);
        int64_t* d = static_cast<int64_t*>(d_out.get());
        check(blsw_r1cs_check_keyset(r1cs_, keys.get(), d, first_unreduced ? d + 1 : nullptr, nullptr), "blsw_r1cs_check_keyset");
        int64_t out[2] = {-1, -1};
        d_out.download(out, first_unreduced ? 16 : 8);
        if (first_unreduced) *first_unreduced = out[1];
        return out[0];
    }
    // cs.is_satisfied() of system i (one check of all n systems per call: call which_is_unsatisfied() once for a whole batch)
    bool is_satisfied(size_t i) {
        if (i >= n_) throw Error("is_satisfied out of range", BLSW_ERR_ARG);
        return which_is_unsatisfied()[i] < 0;
    }
    const blsw_layout_t& layout() const { return layout_; }
    // witness_assignment of system i after verify: n_witness elements of 6 little-endian u64 limbs (Montgomery form: arkworks' in-memory Fq)
    std::vector<uint64_t> witness_assignment(size_t i) const {
        if (!witness_.get() || i >= n_) throw Error("witness_assignment before verify / out of range", BLSW_ERR_ARG);
        std::vector<uint64_t> w((size_t)layout_.n_witness * 6);
        witness_.download(w.data(), w.size() * 8, i * (size_t)layout_.n_witness * 48);
        return w;
    }
    // instance_assignment of system i after verify: n_instance_vars elements (element 0 = one; then the message chunks of UInt8::new_input_vec and
    // the coordinates of the points allocated with AllocationMode::Input, in allocation order), same element encoding as witness_assignment.
    // After aggregate_verify with Input arguments: [1, the keys' x, y, z, the bitmap bits, the message chunks, the signature's six], the Input groups only.
    // After verify_multi with Input arguments: [1, the message chunks pair by pair, the keys' x, y, z pair by pair, the signature's six], likewise
    std::vector<uint64_t> instance_assignment(size_t i) const {
        if (i >= n_) throw Error("instance_assignment out of range", BLSW_ERR_ARG);
        std::vector<uint64_t> v((size_t)layout_.n_instance_vars * 6);
        if (layout_.n_instance_vars == 1 || !instance_.get()) {  // the constant one (R mod p)
            if (layout_.n_instance_vars != 1) throw Error("instance_assignment before verify", BLSW_ERR_ARG);
            const uint64_t one[6] = {0x760900000002fffdull, 0xebf4000bc40c0002ull, 0x5f48985753c758baull, 0x77ce585370525745ull, 0x5c071a97a256ec6dull, 0x15f65ec3fa80e493ull};
            std::memcpy(v.data(), one, 48);
            return v;
        }
        instance_.download(v.data(), v.size() * 8, i * v.size() * 8);
        return v;
    }
    // decode statuses (BLSW_ST_*) of (public key, signature) of system i after verify
    std::array<int32_t, 2> status(size_t i) const { return {status_.at(2 * i), status_.at(2 * i + 1)}; }

   private:
    // check(const KeySet&) hides the namespace's check(rc, what) inside this class: the same function, as an overload of the member
    static void check(int rc, const char* what) { blsw::check(rc, what); }
    friend class ParametersVar;
    friend class UInt8;
    friend class PublicKeyVar;
    friend class SignatureVar;
    friend struct BlsSignatureVerifyGadget;
    size_t n_;
    uint32_t msg_len_;
    int device_;
    blsw_layout_t layout_;
    blsw_engine_t* engine_ = nullptr;
    detail::DeviceBytes workspace_, witness_, instance_, result_, d_status_, pk_xy_, sig_xy_;
    blsw_r1cs_t* r1cs_ = nullptr;  // the device checker (which_is_unsatisfied), built at its first use
    detail::DeviceBytes r1cs_buffer_;
    blsw_matrices_info_t matrices_info() const {
        blsw_matrices_info_t info;
        check(layout_.n_pairs > 1                ? blsw_matrices_info_multi_inputs(msg_len_, layout_.n_pairs, multi_inputs_, &info)
              : layout_.n_keys && agg_inputs_    ? blsw_matrices_info_aggregate_inputs(msg_len_, layout_.n_keys, agg_inputs_, &info)
              : msg_mode_                        ? blsw_matrices_info_inputs(msg_len_, 1, layout_.pk_mode, layout_.sig_mode, &info)
              : layout_.pk_mode || layout_.sig_mode ? blsw_matrices_info_io(msg_len_, layout_.pk_mode, layout_.sig_mode, &info)
              : layout_.params_mode              ? blsw_matrices_info_params(msg_len_, layout_.params_mode, &info)
                                                 : blsw_matrices_info(msg_len_, layout_.n_keys, 1, &info),
              "blsw_matrices_info");
        return info;
    }
    void build_checker() {
        blsw_matrices_info_t info = matrices_info();
        std::vector<uint64_t> rp[3], val[3];
        std::vector<uint32_t> col[3];
        blsw_matrices_t m;
        for (int k = 0; k < 3; k++) {
            rp[k].resize(info.n_constraints + 1);
            col[k].resize(info.nnz[k]);
            val[k].resize(info.nnz[k] * 6);
            m.row_ptr[k] = rp[k].data();
            m.col[k] = col[k].data();
            m.val[k] = val[k].data();
        }
        check(layout_.n_pairs > 1                ? blsw_matrices_fill_multi_inputs(msg_len_, layout_.n_pairs, multi_inputs_, &info, &m)
              : layout_.n_keys && agg_inputs_    ? blsw_matrices_fill_aggregate_inputs(msg_len_, layout_.n_keys, agg_inputs_, &info, &m)
              : msg_mode_                        ? blsw_matrices_fill_inputs(msg_len_, 1, layout_.pk_mode, layout_.sig_mode, &info, &m)
              : layout_.pk_mode || layout_.sig_mode ? blsw_matrices_fill_io(msg_len_, layout_.pk_mode, layout_.sig_mode, &info, &m)
              : layout_.params_mode              ? blsw_matrices_fill_params(msg_len_, layout_.params_mode, &info, &m)
                                                 : blsw_matrices_fill(msg_len_, layout_.n_keys, 1, &info, &m),
              "blsw_matrices_fill");
        uint64_t bytes = 0;
        check(blsw_r1cs_device_bytes(&info, &m, &bytes), "blsw_r1cs_device_bytes");
        r1cs_buffer_ = detail::DeviceBytes(bytes);
        check(blsw_r1cs_create(&r1cs_, &info, &m, device_, r1cs_buffer_.get(), bytes, nullptr), "blsw_r1cs_create");
    }
    // AllocationMode of the message / the key / the signature: part of the circuit shape (blsw_layout_inputs). Each call states all three, so the
    // shape is the same whatever order the new_variable / new_*_vec calls run in.
    void set_io(uint32_t pk_mode, uint32_t sig_mode, uint32_t msg_mode) {
        if (engine_) throw Error("new_variable after verify", BLSW_ERR_ARG);
        if ((pk_mode || sig_mode || msg_mode) && (layout_.params_mode || layout_.n_keys))
            throw Error("AllocationMode::Input: the single-key circuit with Constant parameters", BLSW_ERR_ARG);
        if (pk_mode || sig_mode || msg_mode || layout_.pk_mode || layout_.sig_mode || msg_mode_)
            check(blsw_layout_inputs(msg_len_, msg_mode, pk_mode, sig_mode, &layout_), "blsw_layout_inputs");
        msg_mode_ = msg_mode;
    }
    uint32_t msg_mode_ = 0;  // the message allocated with UInt8::new_input_vec (its chunks are instance_assignment[1 .. c])
    uint32_t agg_inputs_ = 0;  // aggregate_verify: BLSW_AGG_*_INPUT of the circuit it synthesised (blsw_layout_aggregate_inputs)
    uint32_t multi_inputs_ = 0;  // verify_multi: BLSW_MULTI_*_INPUT of the circuit it synthesised (blsw_layout_multi_inputs; layout_.n_pairs > 1)
    std::vector<int32_t> status_;
};

// constraints.rs:341: the message bytes of every system, allocated as witnesses (new_witness_vec: 8 booleans per byte at the head of the vector)
// or as public inputs (new_input_vec: 47-byte chunks as instance variables, each decomposed into 761 witnesses; blsw_layout_inputs)
class MessageVar {
   public:
    const std::vector<uint8_t>& bytes() const { return bytes_; }
    bool is_input() const { return input_; }

   private:
    friend class UInt8;
    std::vector<uint8_t> bytes_;  // [n][msg_len]
    bool input_ = false;
};
class UInt8 {
   public:
    static MessageVar new_witness_vec(ConstraintSystem& cs, const std::vector<std::vector<uint8_t>>& msgs) { return make(cs, msgs, false); }
    // ark-r1cs-std 0.4.0 UInt8::new_input_vec: fixes the message's mode in the circuit shape of `cs`
    static MessageVar new_input_vec(ConstraintSystem& cs, const std::vector<std::vector<uint8_t>>& msgs) {
        MessageVar m = make(cs, msgs, true);
        cs.set_io(cs.layout_.pk_mode, cs.layout_.sig_mode, 1);
        return m;
    }

   private:
    static MessageVar make(ConstraintSystem& cs, const std::vector<std::vector<uint8_t>>& msgs, bool input) {
        if (msgs.size() != cs.num_instances()) throw Error("UInt8::new_*_vec: one message per system", BLSW_ERR_ARG);
        MessageVar m;
        m.input_ = input;
        for (auto& x : msgs) {
            if (x.size() != cs.msg_len()) throw Error("UInt8::new_*_vec: message length != the circuit's", BLSW_ERR_ARG);
            m.bytes_.insert(m.bytes_.end(), x.begin(), x.end());
        }
        return m;
    }
};

// constraints.rs:194-212. Constant (every circuit of the reference) or Witness; fixes the circuit shape of `cs`
class ParametersVar {
   public:
    static ParametersVar new_variable(ConstraintSystem& cs, const Parameters&, AllocationMode mode) {
        if (mode == AllocationMode::Input) throw Error("ParametersVar: AllocationMode::Input (instance variables are not produced)", BLSW_ERR_ARG);
        if (cs.engine_) throw Error("ParametersVar::new_variable after verify", BLSW_ERR_ARG);
        // the allocation modes together fix the circuit shape, whatever the order the three new_variable calls run in (C++ argument evaluation order)
        if (cs.layout_.pk_mode || cs.layout_.sig_mode || cs.msg_mode_) {
            if (mode == AllocationMode::Witness) throw Error("ParametersVar: AllocationMode::Witness together with Input messages / keys / signatures", BLSW_ERR_ARG);
        } else {
            check(blsw_layout_params(cs.msg_len_, mode == AllocationMode::Witness ? 1u : 0u, &cs.layout_), "blsw_layout_params");
        }
        ParametersVar p;
        p.cs_ = &cs;
        return p;
    }

   private:
    friend struct BlsSignatureVerifyGadget;
    ConstraintSystem* cs_ = nullptr;
};
// constraints.rs:214-232 / 234-249: Witness (G1Var / G2Var::new_variable with their in-circuit subgroup checks) or Input (the coordinates are public
// inputs: new_variable_omit_prime_order_check); Constant keys / signatures are a different circuit and not offered
class PublicKeyVar {
   public:
    static PublicKeyVar new_variable(ConstraintSystem& cs, const std::vector<PublicKey>& keys, AllocationMode mode) {
        if (mode == AllocationMode::Constant) throw Error("PublicKeyVar: AllocationMode::Constant is not on the GPU path", BLSW_ERR_ARG);
        if (keys.size() != cs.num_instances()) throw Error("PublicKeyVar::new_variable: one key per system", BLSW_ERR_ARG);
        cs.set_io(mode == AllocationMode::Input ? 1u : 0u, cs.layout_.sig_mode, cs.msg_mode_);
        PublicKeyVar v;
        v.keys_ = keys;
        v.input_ = mode == AllocationMode::Input;
        return v;
    }

   private:
    friend struct BlsSignatureVerifyGadget;
    std::vector<PublicKey> keys_;
    bool input_ = false;
};
class SignatureVar {
   public:
    static SignatureVar new_variable(ConstraintSystem& cs, const std::vector<Signature>& sigs, AllocationMode mode) {
        if (mode == AllocationMode::Constant) throw Error("SignatureVar: AllocationMode::Constant is not on the GPU path", BLSW_ERR_ARG);
        if (sigs.size() != cs.num_instances()) throw Error("SignatureVar::new_variable: one signature per system", BLSW_ERR_ARG);
        cs.set_io(cs.layout_.pk_mode, mode == AllocationMode::Input ? 1u : 0u, cs.msg_mode_);
        SignatureVar v;
        v.sigs_ = sigs;
        v.input_ = mode == AllocationMode::Input;
        return v;
    }

   private:
    friend struct BlsSignatureVerifyGadget;
    std::vector<Signature> sigs_;
    bool input_ = false;
};

// Boolean<ConstraintF>: one Boolean of every system — the gadget's output, or a bitmap entry allocated with new_witness (constraints.rs:414-419) or
// new_input (AllocatedBool::new_variable with Input: a public input that keeps its booleanity constraint and has no witness)
class Boolean {
   public:
    const std::vector<bool>& value() const { return v_; }
    static Boolean new_witness(ConstraintSystem& cs, const std::vector<bool>& values) {
        if (values.size() != cs.num_instances()) throw Error("Boolean::new_witness: one value per system", BLSW_ERR_ARG);
        Boolean b;
        b.v_ = values;
        return b;
    }
    static Boolean new_input(ConstraintSystem& cs, const std::vector<bool>& values) {
        Boolean b = new_witness(cs, values);
        b.input_ = true;
        return b;
    }

   private:
    friend struct BlsSignatureVerifyGadget;
    std::vector<bool> v_;
    bool input_ = false;
};
// UInt32<ConstraintF>: the effective public key count of aggregate_verify (constraints.rs:177-189)
class UInt32 {
   public:
    const std::vector<uint32_t>& value() const { return v_; }

   private:
    friend struct BlsSignatureVerifyGadget;
    std::vector<uint32_t> v_;
};

struct BlsSignatureVerifyGadget {
    // constraints.rs:90-128 for the n systems of `cs`: decodes the keys and signatures, generates every witness of every system on the GPU
    // (blsw_engine_submit_bytes on a direct-mode engine) and returns the output Booleans. Synchronous.
    static Boolean verify(const ParametersVar& parameters, const PublicKeyVar& public_key, const MessageVar& message, const SignatureVar& signature) {
        if (!parameters.cs_) throw Error("verify: parameters were not allocated in a ConstraintSystem", BLSW_ERR_ARG);
        ConstraintSystem& cs = *parameters.cs_;
        const size_t n = cs.n_;
        if (public_key.keys_.size() != n || signature.sigs_.size() != n || message.bytes().size() != n * cs.msg_len_)
            throw Error("verify: variables of another ConstraintSystem", BLSW_ERR_ARG);
        // one circuit shape per ConstraintSystem: aggregate_verify has replaced the layout (num_witness_variables would be the aggregate circuit's)
        if (cs.layout_.n_keys || cs.layout_.n_pairs > 1) throw Error("verify: this ConstraintSystem was synthesised by aggregate_verify / verify_multi; use a new one", BLSW_ERR_ARG);
        if (message.is_input() != (cs.msg_mode_ == 1)) throw Error("verify: the message's AllocationMode is not the one of this ConstraintSystem's circuit", BLSW_ERR_ARG);
        if (!cs.engine_) {
            blsw_engine_options_t opt;
            check(blsw_engine_options_default(&opt), "blsw_engine_options_default");
            opt.device = cs.device_;
            opt.params_mode = cs.layout_.params_mode;
            opt.pk_mode = cs.layout_.pk_mode;
            opt.sig_mode = cs.layout_.sig_mode;
            opt.msg_mode = cs.msg_mode_;
            uint64_t bytes = 0;
            check(blsw_engine_workspace_bytes_ex(n, cs.msg_len_, 1, 1, &opt, &bytes), "blsw_engine_workspace_bytes_ex");
            if (cs.device_ >= 0) hip_check(hipSetDevice(cs.device_), "hipSetDevice");
            cs.workspace_ = detail::DeviceBytes(bytes);
            cs.witness_ = detail::DeviceBytes(n * (size_t)cs.layout_.n_witness * 48);
            cs.instance_ = detail::DeviceBytes(n * (size_t)cs.layout_.n_instance_vars * 48);
            cs.result_ = detail::DeviceBytes(n * 4);
            cs.d_status_ = detail::DeviceBytes(n * 8);
            cs.pk_xy_ = detail::DeviceBytes(n * 96);
            cs.sig_xy_ = detail::DeviceBytes(n * 192);
            check(blsw_engine_create_ex(&cs.engine_, n, cs.msg_len_, 1, 1, &opt, cs.workspace_.get(), bytes), "blsw_engine_create_ex");
        }
        std::vector<uint8_t> pk(n * 48), sg(n * 96);
        for (size_t i = 0; i < n; i++) {
            std::memcpy(&pk[48 * i], public_key.keys_[i].bytes.data(), 48);
            std::memcpy(&sg[96 * i], signature.sigs_[i].bytes.data(), 96);
        }
        detail::DeviceBytes d_pk(pk.size()), d_sg(sg.size()), d_msg(message.bytes().size());
        d_pk.upload(pk.data(), pk.size());
        d_sg.upload(sg.data(), sg.size());
        if (!message.bytes().empty()) d_msg.upload(message.bytes().data(), message.bytes().size());
        const bool io = cs.layout_.pk_mode || cs.layout_.sig_mode || cs.msg_mode_;
        if (io) {  // public inputs: decode, then the step that also writes instance_assignment; the fallback rule of tests/tests.rs:244-263 is applied below
            check(blsw_decode_batch(static_cast<const uint8_t*>(d_pk.get()), static_cast<const uint8_t*>(d_sg.get()), n, static_cast<uint64_t*>(cs.pk_xy_.get()),
                                    static_cast<uint64_t*>(cs.sig_xy_.get()), static_cast<int32_t*>(cs.d_status_.get()), nullptr),
                  "blsw_decode_batch");
            check(blsw_engine_submit_io(cs.engine_, static_cast<const uint64_t*>(cs.pk_xy_.get()), static_cast<const uint64_t*>(cs.sig_xy_.get()),
                                        static_cast<const uint8_t*>(d_msg.get()), static_cast<uint64_t*>(cs.instance_.get()), static_cast<uint64_t*>(cs.witness_.get()),
                                        cs.layout_.n_witness, static_cast<int32_t*>(cs.result_.get()), nullptr),
                  "blsw_engine_submit_io");
        } else {
            check(blsw_engine_submit_bytes(cs.engine_, static_cast<const uint8_t*>(d_pk.get()), static_cast<const uint8_t*>(d_sg.get()),
                                           static_cast<const uint8_t*>(d_msg.get()), static_cast<uint64_t*>(cs.pk_xy_.get()), static_cast<uint64_t*>(cs.sig_xy_.get()),
                                           static_cast<int32_t*>(cs.d_status_.get()), static_cast<uint64_t*>(cs.witness_.get()), cs.layout_.n_witness,
                                           static_cast<int32_t*>(cs.result_.get()), nullptr),
                  "blsw_engine_submit_bytes");
        }
        check(blsw_engine_flush(cs.engine_, nullptr), "blsw_engine_flush");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        std::vector<int32_t> r(n);
        cs.result_.download(r.data(), n * 4);
        cs.status_.resize(2 * n);
        cs.d_status_.download(cs.status_.data(), n * 8);
        if (io)
            for (size_t i = 0; i < n; i++)
                if (cs.status_[2 * i] | cs.status_[2 * i + 1]) r[i] = 0;
        Boolean b;
        b.v_.resize(n);
        for (size_t i = 0; i < n; i++) b.v_[i] = r[i] == 1;
        return b;
    }

    // constraints.rs:153-167 for the n systems of `cs`: public_keys[k] / bitmap[k] hold key k / bit k of every system (the reference passes
    // slices of K variables of one system). Returns (result, effective public key count). The circuit is the one of blsw_layout_aggregate:
    // keys, bitmap, msg, sig allocated in the order of constraints.rs:378-441, Constant parameters. A key that FAILS TO DECODE (bad encoding,
    // not on the curve, not in the subgroup) or a signature that does not decode to a non-identity point makes its system false (status()),
    // as in verify. The infinity encoding of a KEY decodes (PublicKey::try_from accepts it, and a key whose bitmap bit is 0 never enters
    // the aggregate, constraints.rs:169-191): such a system returns the gadget's own Boolean. Synchronous; direct-mode batch entry
    // blsw_aggregate_verify_batch.
    // Each argument may be allocated as Input instead (PublicKeyVar / SignatureVar::new_variable(.., Input), Boolean::new_input,
    // UInt8::new_input_vec; all keys in one mode, all bits in one mode): the circuit is then the one of blsw_layout_aggregate_inputs, run by a
    // direct-mode engine with options.agg_inputs, and instance_assignment(i) holds the public inputs.
    static std::pair<Boolean, UInt32> aggregate_verify(const ParametersVar& parameters, const std::vector<PublicKeyVar>& public_keys, const std::vector<Boolean>& bitmap,
                                                       const MessageVar& message, const SignatureVar& signature) {
        if (!parameters.cs_) throw Error("aggregate_verify: parameters were not allocated in a ConstraintSystem", BLSW_ERR_ARG);
        ConstraintSystem& cs = *parameters.cs_;
        const size_t n = cs.n_, K = public_keys.size();
        if (K == 0 || bitmap.size() != K) throw Error("aggregate_verify: public_keys.len() == bitmap.len() > 0", BLSW_ERR_ARG);  // constraints.rs:160
        if (cs.layout_.params_mode || cs.engine_) throw Error("aggregate_verify: Constant parameters, a ConstraintSystem not used by verify", BLSW_ERR_ARG);
        if (signature.sigs_.size() != n || message.bytes().size() != n * cs.msg_len_) throw Error("aggregate_verify: variables of another ConstraintSystem", BLSW_ERR_ARG);
        for (size_t k = 1; k < K; k++)
            if (public_keys[k].input_ != public_keys[0].input_ || bitmap[k].input_ != bitmap[0].input_)
                throw Error("aggregate_verify: every key in one AllocationMode, every bitmap bit in one AllocationMode", BLSW_ERR_ARG);
        const uint32_t mask = (public_keys[0].input_ ? BLSW_AGG_KEYS_INPUT : 0u) | (bitmap[0].input_ ? BLSW_AGG_BITMAP_INPUT : 0u) |
                              (message.is_input() ? BLSW_AGG_MSG_INPUT : 0u) | (signature.input_ ? BLSW_AGG_SIG_INPUT : 0u);
        cs.agg_inputs_ = mask;
        cs.msg_mode_ = 0;  // the aggregate circuit's modes are the mask
        check(mask ? blsw_layout_aggregate_inputs(cs.msg_len_, (uint32_t)K, mask, &cs.layout_) : blsw_layout_aggregate(cs.msg_len_, (uint32_t)K, &cs.layout_),
              "blsw_layout_aggregate");
        if (cs.device_ >= 0) hip_check(hipSetDevice(cs.device_), "hipSetDevice");
        // compressed inputs, system-major: keys [n][K][48], bitmap [n][K], signatures [n][96]
        std::vector<uint8_t> pk(n * K * 48), bm(n * K), sg(n * 96);
        for (size_t k = 0; k < K; k++) {
            if (public_keys[k].keys_.size() != n || bitmap[k].v_.size() != n) throw Error("aggregate_verify: one key and one bit per system", BLSW_ERR_ARG);
            for (size_t i = 0; i < n; i++) {
                std::memcpy(&pk[(i * K + k) * 48], public_keys[k].keys_[i].bytes.data(), 48);
                bm[i * K + k] = bitmap[k].v_[i] ? 1 : 0;
            }
        }
        for (size_t i = 0; i < n; i++) std::memcpy(&sg[96 * i], signature.sigs_[i].bytes.data(), 96);
        // decode (blsw_decode_batch takes as many keys as signatures: the keys with a block of zero bytes beside them, then the signatures likewise)
        const size_t m = n * K;
        detail::DeviceBytes d_pk(m * 48), d_sg(m * 96), d_pk_xy(m * 96), d_sg_xy(m * 192), d_st(m * 8), d_bm(m), d_msg(message.bytes().size());
        hip_check(hipMemset(d_sg.get(), 0, m * 96), "hipMemset");
        d_pk.upload(pk.data(), pk.size());
        check(blsw_decode_batch(static_cast<const uint8_t*>(d_pk.get()), static_cast<const uint8_t*>(d_sg.get()), m, static_cast<uint64_t*>(d_pk_xy.get()),
                                static_cast<uint64_t*>(d_sg_xy.get()), static_cast<int32_t*>(d_st.get()), nullptr),
              "blsw_decode_batch");
        std::vector<int32_t> st_keys(2 * m);
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        d_st.download(st_keys.data(), m * 8);
        detail::DeviceBytes d_pk0(n * 48), d_sig(n * 96), d_pk0_xy(n * 96), d_st2(n * 8);
        cs.sig_xy_ = detail::DeviceBytes(n * 192);
        hip_check(hipMemset(d_pk0.get(), 0, n * 48), "hipMemset");
        d_sig.upload(sg.data(), sg.size());
        check(blsw_decode_batch(static_cast<const uint8_t*>(d_pk0.get()), static_cast<const uint8_t*>(d_sig.get()), n, static_cast<uint64_t*>(d_pk0_xy.get()),
                                static_cast<uint64_t*>(cs.sig_xy_.get()), static_cast<int32_t*>(d_st2.get()), nullptr),
              "blsw_decode_batch");
        std::vector<int32_t> st_sig(2 * n);
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        d_st2.download(st_sig.data(), n * 8);
        d_bm.upload(bm.data(), bm.size());
        if (!message.bytes().empty()) d_msg.upload(message.bytes().data(), message.bytes().size());
        uint64_t bytes = 0;
        detail::DeviceBytes d_count(n * 4);
        cs.witness_ = detail::DeviceBytes(n * (size_t)cs.layout_.n_witness * 48);
        cs.result_ = detail::DeviceBytes(n * 4);
        if (mask) {  // a direct-mode engine of the circuit with these Input arguments; the step also writes instance_assignment
            blsw_engine_options_t opt;
            check(blsw_engine_options_default(&opt), "blsw_engine_options_default");
            opt.device = cs.device_;
            opt.n_keys = (uint32_t)K;
            opt.agg_inputs = mask;
            check(blsw_engine_workspace_bytes_ex(n, cs.msg_len_, 1, 1, &opt, &bytes), "blsw_engine_workspace_bytes_ex");
            cs.workspace_ = detail::DeviceBytes(bytes);
            cs.instance_ = detail::DeviceBytes(n * (size_t)cs.layout_.n_instance_vars * 48);
            cs.pk_xy_ = std::move(d_pk_xy);  // the step's inputs stay alive with the system
            check(blsw_engine_create_ex(&cs.engine_, n, cs.msg_len_, 1, 1, &opt, cs.workspace_.get(), bytes), "blsw_engine_create_ex");
            check(blsw_engine_submit_aggregate_io(cs.engine_, static_cast<const uint64_t*>(cs.pk_xy_.get()), static_cast<const uint8_t*>(d_bm.get()),
                                                  static_cast<const uint64_t*>(cs.sig_xy_.get()), static_cast<const uint8_t*>(d_msg.get()),
                                                  static_cast<uint64_t*>(cs.instance_.get()), static_cast<uint64_t*>(cs.witness_.get()), cs.layout_.n_witness,
                                                  static_cast<int32_t*>(cs.result_.get()), static_cast<uint32_t*>(d_count.get()), nullptr),
                  "blsw_engine_submit_aggregate_io");
            check(blsw_engine_flush(cs.engine_, nullptr), "blsw_engine_flush");
        } else {
        check(blsw_aggregate_workspace_bytes(n, cs.msg_len_, (uint32_t)K, &bytes), "blsw_aggregate_workspace_bytes");
        cs.workspace_ = detail::DeviceBytes(bytes);
        check(blsw_aggregate_verify_batch(static_cast<const uint64_t*>(d_pk_xy.get()), static_cast<const uint8_t*>(d_bm.get()), (uint32_t)K,
                                          static_cast<const uint64_t*>(cs.sig_xy_.get()), static_cast<const uint8_t*>(d_msg.get()), cs.msg_len_, n,
                                          static_cast<uint64_t*>(cs.witness_.get()), cs.layout_.n_witness, static_cast<int32_t*>(cs.result_.get()),
                                          static_cast<uint32_t*>(d_count.get()), cs.workspace_.get(), bytes, nullptr),
              "blsw_aggregate_verify_batch");
        }
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        std::vector<int32_t> r(n);
        cs.result_.download(r.data(), n * 4);
        UInt32 count;
        count.v_.resize(n);
        d_count.download(count.v_.data(), n * 4);
        // status(i): the first key of system i that failed to decode (else OK: a well-formed identity key is not a failure), and the signature's
        cs.status_.assign(2 * n, BLSW_ST_OK);
        Boolean b;
        b.v_.resize(n);
        for (size_t i = 0; i < n; i++) {
            for (size_t k = 0; k < K && cs.status_[2 * i] == BLSW_ST_OK; k++) {
                const int32_t st = st_keys[2 * (i * K + k)];
                if (st != BLSW_ST_IDENTITY) cs.status_[2 * i] = st;
            }
            cs.status_[2 * i + 1] = st_sig[2 * i + 1];
            b.v_[i] = r[i] == 1 && cs.status_[2 * i] == BLSW_ST_OK && cs.status_[2 * i + 1] == BLSW_ST_OK;
        }
        return {b, count};
    }

    // The N+1-pair product (blsw_layout_multi) for the n systems of `cs`: ONE signature over K (pk_j, msg_j) pairs per system; public_keys[j] /
    // messages[j] hold key j / message j of every system. K >= 2, Constant parameters. The keys (all in one mode), the messages (all in one mode) and
    // the signature may each be allocated as Input (PublicKeyVar / SignatureVar::new_variable(.., Input), UInt8::new_input_vec): the circuit is the
    // one of blsw_layout_multi_inputs, and instance_assignment(i) holds the public inputs. Runs on an engine of blsw_engine_create_multi_inputs with options.n_pairs = K (one step per
    // group, two group buffers). A key or a signature that does not decode to a non-identity subgroup point makes its system false (status(): the
    // first such key's status, the signature's), as in verify. Synchronous.
    static Boolean verify_multi(const ParametersVar& parameters, const std::vector<PublicKeyVar>& public_keys, const std::vector<MessageVar>& messages,
                                const SignatureVar& signature) {
        if (!parameters.cs_) throw Error("verify_multi: parameters were not allocated in a ConstraintSystem", BLSW_ERR_ARG);
        ConstraintSystem& cs = *parameters.cs_;
        const size_t n = cs.n_, K = public_keys.size();
        if (K < 2 || messages.size() != K) throw Error("verify_multi: public_keys.len() == messages.len() >= 2", BLSW_ERR_ARG);
        if (cs.layout_.params_mode || cs.engine_) throw Error("verify_multi: Constant parameters, a ConstraintSystem not used by verify", BLSW_ERR_ARG);
        if (signature.sigs_.size() != n) throw Error("verify_multi: variables of another ConstraintSystem", BLSW_ERR_ARG);
        for (size_t j = 0; j < K; j++) {
            if (public_keys[j].keys_.size() != n || messages[j].bytes().size() != n * cs.msg_len_) throw Error("verify_multi: one key and one message per pair and system", BLSW_ERR_ARG);
            if (public_keys[j].input_ != public_keys[0].input_ || messages[j].is_input() != messages[0].is_input())
                throw Error("verify_multi: every key in one AllocationMode, every message in one AllocationMode", BLSW_ERR_ARG);
        }
        const uint32_t mask = (public_keys[0].input_ ? BLSW_MULTI_KEYS_INPUT : 0u) | (messages[0].is_input() ? BLSW_MULTI_MSG_INPUT : 0u) |
                              (signature.input_ ? BLSW_MULTI_SIG_INPUT : 0u);
        cs.multi_inputs_ = mask;
        cs.msg_mode_ = 0;  // the product's modes are the mask
        check(blsw_layout_multi_inputs(cs.msg_len_, (uint32_t)K, mask, &cs.layout_), "blsw_layout_multi_inputs");
        if (cs.device_ >= 0) hip_check(hipSetDevice(cs.device_), "hipSetDevice");
        // compressed inputs, system-major: keys [n][K][48], messages [n][K][msg_len], signatures [n][96]
        const size_t m = n * K, len = cs.msg_len_;
        std::vector<uint8_t> pk(m * 48), msg(m * len), sg(n * 96);
        for (size_t j = 0; j < K; j++)
            for (size_t i = 0; i < n; i++) {
                std::memcpy(&pk[(i * K + j) * 48], public_keys[j].keys_[i].bytes.data(), 48);
                if (len) std::memcpy(&msg[(i * K + j) * len], &messages[j].bytes()[i * len], len);
            }
        for (size_t i = 0; i < n; i++) std::memcpy(&sg[96 * i], signature.sigs_[i].bytes.data(), 96);
        // decode (blsw_decode_batch takes as many keys as signatures: the keys with a block of zero bytes beside them, then the signatures likewise)
        detail::DeviceBytes d_pk(m * 48), d_sg(m * 96), d_sg_xy(m * 192), d_st(m * 8), d_msg(msg.size());
        cs.pk_xy_ = detail::DeviceBytes(m * 96);  // the step's inputs stay alive with the system
        hip_check(hipMemset(d_sg.get(), 0, m * 96), "hipMemset");
        d_pk.upload(pk.data(), pk.size());
        check(blsw_decode_batch(static_cast<const uint8_t*>(d_pk.get()), static_cast<const uint8_t*>(d_sg.get()), m, static_cast<uint64_t*>(cs.pk_xy_.get()),
                                static_cast<uint64_t*>(d_sg_xy.get()), static_cast<int32_t*>(d_st.get()), nullptr),
              "blsw_decode_batch");
        std::vector<int32_t> st_keys(2 * m);
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        d_st.download(st_keys.data(), m * 8);
        detail::DeviceBytes d_pk0(n * 48), d_sig(n * 96), d_pk0_xy(n * 96), d_st2(n * 8);
        cs.sig_xy_ = detail::DeviceBytes(n * 192);
        hip_check(hipMemset(d_pk0.get(), 0, n * 48), "hipMemset");
        d_sig.upload(sg.data(), sg.size());
        check(blsw_decode_batch(static_cast<const uint8_t*>(d_pk0.get()), static_cast<const uint8_t*>(d_sig.get()), n, static_cast<uint64_t*>(d_pk0_xy.get()),
                                static_cast<uint64_t*>(cs.sig_xy_.get()), static_cast<int32_t*>(d_st2.get()), nullptr),
              "blsw_decode_batch");
        std::vector<int32_t> st_sig(2 * n);
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        d_st2.download(st_sig.data(), n * 8);
        if (!msg.empty()) d_msg.upload(msg.data(), msg.size());
        blsw_engine_options_t opt;
        check(blsw_engine_options_default(&opt), "blsw_engine_options_default");
        opt.device = cs.device_;
        opt.n_pairs = (uint32_t)K;
        uint64_t bytes = 0;
        check(blsw_engine_workspace_bytes_multi_inputs(n, cs.msg_len_, 1, 2, &opt, mask, &bytes), "blsw_engine_workspace_bytes_multi_inputs");
        cs.workspace_ = detail::DeviceBytes(bytes);
        cs.witness_ = detail::DeviceBytes(n * (size_t)cs.layout_.n_witness * 48);
        cs.instance_ = detail::DeviceBytes(n * (size_t)cs.layout_.n_instance_vars * 48);
        cs.result_ = detail::DeviceBytes(n * 4);
        check(blsw_engine_create_multi_inputs(&cs.engine_, n, cs.msg_len_, 1, 2, &opt, mask, cs.workspace_.get(), bytes), "blsw_engine_create_multi_inputs");
        check(blsw_engine_submit_multi_io(cs.engine_, static_cast<const uint64_t*>(cs.pk_xy_.get()), static_cast<const uint8_t*>(d_msg.get()),
                                          static_cast<const uint64_t*>(cs.sig_xy_.get()), static_cast<uint64_t*>(cs.instance_.get()),
                                          static_cast<uint64_t*>(cs.witness_.get()), cs.layout_.n_witness, static_cast<int32_t*>(cs.result_.get()), nullptr),
              "blsw_engine_submit_multi_io");
        check(blsw_engine_flush(cs.engine_, nullptr), "blsw_engine_flush");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        std::vector<int32_t> r(n);
        cs.result_.download(r.data(), n * 4);
        cs.status_.assign(2 * n, BLSW_ST_OK);
        Boolean b;
        b.v_.resize(n);
        for (size_t i = 0; i < n; i++) {
            for (size_t j = 0; j < K && cs.status_[2 * i] == BLSW_ST_OK; j++) cs.status_[2 * i] = st_keys[2 * (i * K + j)];
            cs.status_[2 * i + 1] = st_sig[2 * i + 1];
            b.v_[i] = r[i] == 1 && cs.status_[2 * i] == BLSW_ST_OK && cs.status_[2 * i + 1] == BLSW_ST_OK;
        }
        return b;
    }
};

// The domain separation tag of hash_to_curve for the BLS:: value functions (blsw_dst_t, include/blsw.h): 1 .. 255 bytes. A default-constructed Dst
// is "the library's tag through the plain entry" (get() == nullptr); Dst::pop() is the proof-of-possession tag of the signature draft.
class Dst {
public:
    Dst() = default;
    explicit Dst(const std::string& tag) : set_(true) { check(blsw_dst_set(&t_, reinterpret_cast<const uint8_t*>(tag.data()), (uint32_t)tag.size()), "blsw_dst_set"); }
    explicit Dst(const std::vector<uint8_t>& tag) : set_(true) { check(blsw_dst_set(&t_, tag.data(), (uint32_t)tag.size()), "blsw_dst_set"); }
    static Dst library() {
        Dst d;
        d.set_ = true;
        check(blsw_dst_default(&d.t_), "blsw_dst_default");
        return d;
    }
    static Dst pop() {
        Dst d;
        d.set_ = true;
        check(blsw_dst_pop(&d.t_), "blsw_dst_pop");
        return d;
    }
    const blsw_dst_t* get() const { return set_ ? &t_ : nullptr; }
    std::vector<uint8_t> bytes() const { return set_ ? std::vector<uint8_t>(t_.bytes, t_.bytes + t_.len) : Dst::library().bytes(); }

private:
    blsw_dst_t t_{};
    bool set_ = false;
};

// The native scheme (src/bls.rs:395-458, `impl SignatureScheme for BLS`) for batches: one secret key / message / signature per element.
// Every function takes the tag as its last argument: the default is the library's (the plain C entry, exactly as before).
struct SecretKey {
    std::array<uint8_t, 32> le;  // PrivateKey::try_from(&[u8]) (bls.rs:97-103): little-endian Fr
    static SecretKey try_from(const std::string& hex_be) {  // the fixtures' big-endian hex ("0x..." allowed)
        SecretKey k;
        auto b = detail::unhex(hex_be, 32);
        for (int i = 0; i < 32; i++) k.le[i] = b[31 - i];
        return k;
    }
};
struct BLS {
    struct Signed {
        std::vector<Signature> signatures;    // Signature (compressed), the infinity encoding where status != BLSW_ST_OK
        std::vector<PublicKey> public_keys;   // PublicKey::from(&sk)
        std::vector<int32_t> status;          // BLSW_ST_OK, BLSW_ST_INVALID_SECRET_KEY (sk = 0: Err(InvalidSecretKey), bls.rs:417-419), BLSW_ST_BAD_ENCODING (sk >= r)
    };
    // BLS::sign (bls.rs:411-425) and PublicKey::from(&sk) (bls.rs:183-195): messages [n][msg_len]
    static Signed sign(const Parameters&, const std::vector<SecretKey>& sks, const std::vector<std::vector<uint8_t>>& messages, const Dst& dst = Dst()) {
        const size_t n = sks.size();
        if (n == 0 || messages.size() != n) throw Error("BLS::sign: one message per key", BLSW_ERR_ARG);
        const uint32_t msg_len = (uint32_t)messages[0].size();
        std::vector<uint8_t> sk(n * 32), msg(n * (size_t)msg_len);
        for (size_t i = 0; i < n; i++) {
            if (messages[i].size() != msg_len) throw Error("BLS::sign: messages of one length per batch", BLSW_ERR_ARG);
            std::memcpy(&sk[32 * i], sks[i].le.data(), 32);
            if (msg_len) std::memcpy(&msg[(size_t)msg_len * i], messages[i].data(), msg_len);
        }
        uint64_t bytes = 0;
        check(blsw_hash_to_g2_workspace_bytes(n, msg_len, &bytes), "blsw_hash_to_g2_workspace_bytes");
        detail::DeviceBytes d_sk(sk.size()), d_msg(msg.size()), d_sig(n * 96), d_pk(n * 48), d_st(n * 4), ws(bytes);
        d_sk.upload(sk.data(), sk.size());
        if (!msg.empty()) d_msg.upload(msg.data(), msg.size());
        check(blsw_sign_batch_dst(static_cast<const uint8_t*>(d_sk.get()), static_cast<const uint8_t*>(d_msg.get()), msg_len, n, static_cast<uint8_t*>(d_sig.get()), nullptr,
                              static_cast<uint8_t*>(d_pk.get()), nullptr, static_cast<int32_t*>(d_st.get()), ws.get(), bytes, dst.get(), nullptr),
              "blsw_sign_batch");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        std::vector<uint8_t> sg(n * 96), pk(n * 48);
        Signed out;
        out.status.resize(n);
        d_sig.download(sg.data(), sg.size());
        d_pk.download(pk.data(), pk.size());
        d_st.download(out.status.data(), n * 4);
        out.signatures.resize(n);
        out.public_keys.resize(n);
        for (size_t i = 0; i < n; i++) {
            std::memcpy(out.signatures[i].bytes.data(), &sg[96 * i], 96);
            std::memcpy(out.public_keys[i].bytes.data(), &pk[48 * i], 48);
        }
        return out;
    }
    // BLS::verify (bls.rs:427-458) for n (pk, msg, sig) triples: the native pairing check as values (no circuit, no witness tensor).
    // An identity or undecodable key / signature is Err(..) in the reference and `false` here, with the reason in `status` ([n][2], BLSW_ST_*).
    static std::vector<bool> verify(const Parameters&, const std::vector<PublicKey>& pks, const std::vector<std::vector<uint8_t>>& messages,
                                    const std::vector<Signature>& sigs, std::vector<int32_t>* status = nullptr, const Dst& dst = Dst()) {
        const size_t n = pks.size();
        if (n == 0 || messages.size() != n || sigs.size() != n) throw Error("BLS::verify: one message and one signature per key", BLSW_ERR_ARG);
        const uint32_t msg_len = (uint32_t)messages[0].size();
        std::vector<uint8_t> pk(n * 48), sg(n * 96), msg(n * (size_t)msg_len);
        for (size_t i = 0; i < n; i++) {
            if (messages[i].size() != msg_len) throw Error("BLS::verify: messages of one length per batch", BLSW_ERR_ARG);
            std::memcpy(&pk[48 * i], pks[i].bytes.data(), 48);
            std::memcpy(&sg[96 * i], sigs[i].bytes.data(), 96);
            if (msg_len) std::memcpy(&msg[(size_t)msg_len * i], messages[i].data(), msg_len);
        }
        uint64_t bytes = 0;
        check(blsw_verify_workspace_bytes(n, msg_len, &bytes), "blsw_verify_workspace_bytes");
        detail::DeviceBytes ws(bytes), d_pk(pk.size()), d_sg(sg.size()), d_msg(msg.size()), d_st(n * 8), d_res(n * 4);
        d_pk.upload(pk.data(), pk.size());
        d_sg.upload(sg.data(), sg.size());
        if (!msg.empty()) d_msg.upload(msg.data(), msg.size());
        // the native algorithm as values (blsw_verify_batch): decode + subgroup checks, hash to G2, projective two-pair Miller loop, final exponentiation
        check(blsw_verify_batch_dst(static_cast<const uint8_t*>(d_pk.get()), static_cast<const uint8_t*>(d_sg.get()), static_cast<const uint8_t*>(d_msg.get()), msg_len, n,
                                static_cast<int32_t*>(d_res.get()), static_cast<int32_t*>(d_st.get()), ws.get(), bytes, dst.get(), nullptr),
              "blsw_verify_batch");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        std::vector<int32_t> r(n);
        d_res.download(r.data(), n * 4);
        if (status) {
            status->resize(2 * n);
            d_st.download(status->data(), n * 8);
        }
        std::vector<bool> out(n);
        for (size_t i = 0; i < n; i++) out[i] = r[i] == 1;
        return out;
    }
    // n fresh 64-bit coefficients from the operating system's generator, none of them zero (what verify_groups draws when given none)
    static std::vector<uint64_t> group_scalars(size_t n) {
        std::random_device rd;
        std::vector<uint64_t> r(n);
        for (auto& v : r) {
            v = ((uint64_t)rd() << 32) ^ (uint64_t)rd();
            if (v == 0) v = 1;
        }
        return r;
    }
    // Groups of triples verified with random coefficients (blsw_verify_groups_batch, include/blsw.h): verdict j is for triples
    // [j * group, min(n, (j + 1) * group)) — true iff every triple decodes, every coefficient is non-zero and the group's product of pairings is one.
    // scalars: empty draws group_scalars(n); given ones are used as they are, and predictable ones are NOT sound (include/blsw.h, P4).
    static std::vector<bool> verify_groups(const Parameters&, const std::vector<PublicKey>& pks, const std::vector<std::vector<uint8_t>>& messages,
                                           const std::vector<Signature>& sigs, uint32_t group = 64, std::vector<uint64_t> scalars = {},
                                           std::vector<int32_t>* status = nullptr, const Dst& dst = Dst()) {
        const size_t n = pks.size();
        if (n == 0 || messages.size() != n || sigs.size() != n || group == 0) throw Error("BLS::verify_groups: one message and one signature per key", BLSW_ERR_ARG);
        if (scalars.empty()) scalars = group_scalars(n);
        if (scalars.size() != n) throw Error("BLS::verify_groups: one coefficient per triple", BLSW_ERR_ARG);
        const uint32_t msg_len = (uint32_t)messages[0].size();
        std::vector<uint8_t> pk(n * 48), sg(n * 96), msg(n * (size_t)msg_len);
        for (size_t i = 0; i < n; i++) {
            if (messages[i].size() != msg_len) throw Error("BLS::verify_groups: messages of one length per batch", BLSW_ERR_ARG);
            std::memcpy(&pk[48 * i], pks[i].bytes.data(), 48);
            std::memcpy(&sg[96 * i], sigs[i].bytes.data(), 96);
            if (msg_len) std::memcpy(&msg[(size_t)msg_len * i], messages[i].data(), msg_len);
        }
        const size_t n_groups = (n + group - 1) / group;
        uint64_t bytes = 0;
        check(blsw_verify_groups_workspace_bytes(n, msg_len, group, &bytes), "blsw_verify_groups_workspace_bytes");
        detail::DeviceBytes ws(bytes), d_pk(pk.size()), d_sg(sg.size()), d_msg(msg.size()), d_sc(n * 8), d_st(n * 8), d_res(n_groups * 4);
        d_pk.upload(pk.data(), pk.size());
        d_sg.upload(sg.data(), sg.size());
        d_sc.upload(scalars.data(), n * 8);
        if (!msg.empty()) d_msg.upload(msg.data(), msg.size());
        check(blsw_verify_groups_batch_dst(static_cast<const uint8_t*>(d_pk.get()), static_cast<const uint8_t*>(d_sg.get()), static_cast<const uint8_t*>(d_msg.get()), msg_len, n,
                                       static_cast<const uint64_t*>(d_sc.get()), group, static_cast<int32_t*>(d_res.get()), static_cast<int32_t*>(d_st.get()), ws.get(), bytes,
                                       dst.get(), nullptr),
              "blsw_verify_groups_batch");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        std::vector<int32_t> r(n_groups);
        d_res.download(r.data(), n_groups * 4);
        if (status) {
            status->resize(2 * n);
            d_st.download(status->data(), n * 8);
        }
        std::vector<bool> out(n_groups);
        for (size_t j = 0; j < n_groups; j++) out[j] = r[j] == 1;
        return out;
    }
    // verify_groups over a message TABLE (blsw_verify_groups_shared_batch, include/blsw.h): triple i signs table[msg_index[i]]. One hash per table row
    // and one pair per run of equal adjacent indices of a group — sort each group by index. An index beyond the table is BLSW_ST_BAD_INDEX in
    // status[2 i] and fails its group. runs (when given) receives the number of runs of each group; everything else as verify_groups.
    static std::vector<bool> verify_groups_shared(const Parameters&, const std::vector<PublicKey>& pks, const std::vector<std::vector<uint8_t>>& table,
                                                  const std::vector<uint32_t>& msg_index, const std::vector<Signature>& sigs, uint32_t group = 64,
                                                  std::vector<uint64_t> scalars = {}, std::vector<int32_t>* status = nullptr, std::vector<uint32_t>* runs = nullptr,
                                                  const Dst& dst = Dst()) {
        const size_t n = pks.size(), n_msgs = table.size();
        if (n == 0 || n_msgs == 0 || msg_index.size() != n || sigs.size() != n || group == 0)
            throw Error("BLS::verify_groups_shared: a table, and one index and one signature per key", BLSW_ERR_ARG);
        if (scalars.empty()) scalars = group_scalars(n);
        if (scalars.size() != n) throw Error("BLS::verify_groups_shared: one coefficient per triple", BLSW_ERR_ARG);
        const uint32_t msg_len = (uint32_t)table[0].size();
        std::vector<uint8_t> pk(n * 48), sg(n * 96), msg(n_msgs * (size_t)msg_len);
        for (size_t i = 0; i < n; i++) {
            std::memcpy(&pk[48 * i], pks[i].bytes.data(), 48);
            std::memcpy(&sg[96 * i], sigs[i].bytes.data(), 96);
        }
        for (size_t r = 0; r < n_msgs; r++) {
            if (table[r].size() != msg_len) throw Error("BLS::verify_groups_shared: messages of one length per table", BLSW_ERR_ARG);
            if (msg_len) std::memcpy(&msg[(size_t)msg_len * r], table[r].data(), msg_len);
        }
        const size_t n_groups = (n + group - 1) / group;
        uint64_t bytes = 0;
        check(blsw_verify_groups_shared_workspace_bytes(n, n_msgs, msg_len, group, &bytes), "blsw_verify_groups_shared_workspace_bytes");
        detail::DeviceBytes ws(bytes), d_pk(pk.size()), d_sg(sg.size()), d_msg(msg.size()), d_ix(n * 4), d_sc(n * 8), d_st(n * 8), d_res(n_groups * 4), d_runs(n_groups * 4);
        d_pk.upload(pk.data(), pk.size());
        d_sg.upload(sg.data(), sg.size());
        d_ix.upload(msg_index.data(), n * 4);
        d_sc.upload(scalars.data(), n * 8);
        if (!msg.empty()) d_msg.upload(msg.data(), msg.size());
        check(blsw_verify_groups_shared_batch(static_cast<const uint8_t*>(d_pk.get()), static_cast<const uint8_t*>(d_sg.get()), static_cast<const uint8_t*>(d_msg.get()), msg_len, n_msgs,
                                              static_cast<const uint32_t*>(d_ix.get()), n, static_cast<const uint64_t*>(d_sc.get()), group, dst.get(),
                                              static_cast<int32_t*>(d_res.get()), static_cast<uint32_t*>(d_runs.get()), static_cast<int32_t*>(d_st.get()), ws.get(), bytes, nullptr),
              "blsw_verify_groups_shared_batch");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        std::vector<int32_t> r(n_groups);
        d_res.download(r.data(), n_groups * 4);
        if (status) {
            status->resize(2 * n);
            d_st.download(status->data(), n * 8);
        }
        if (runs) {
            runs->resize(n_groups);
            d_runs.download(runs->data(), n_groups * 4);
        }
        std::vector<bool> out(n_groups);
        for (size_t j = 0; j < n_groups; j++) out[j] = r[j] == 1;
        return out;
    }
    // BLS::verify through verify_groups: the triples of passing groups are true, those of failing groups go through verify once more. A batch in which
    // most groups hold a bad triple is slower this way than verify.
    static std::vector<bool> verify_grouped(const Parameters& params, const std::vector<PublicKey>& pks, const std::vector<std::vector<uint8_t>>& messages,
                                            const std::vector<Signature>& sigs, uint32_t group = 64, std::vector<uint64_t> scalars = {},
                                            std::vector<int32_t>* status = nullptr, const Dst& dst = Dst()) {
        const std::vector<bool> g = verify_groups(params, pks, messages, sigs, group, std::move(scalars), status, dst);
        const size_t n = pks.size();
        std::vector<bool> out(n, true);
        std::vector<size_t> idx;
        for (size_t i = 0; i < n; i++)
            if (!g[i / group]) idx.push_back(i);
        if (idx.empty()) return out;
        std::vector<PublicKey> p2;
        std::vector<std::vector<uint8_t>> m2;
        std::vector<Signature> s2;
        for (size_t i : idx) {
            p2.push_back(pks[i]);
            m2.push_back(messages[i]);
            s2.push_back(sigs[i]);
        }
        const std::vector<bool> r = verify(params, p2, m2, s2, nullptr, dst);
        for (size_t k = 0; k < idx.size(); k++) out[idx[k]] = r[k];
        return out;
    }
    // fast_aggregate_verify (tests/tests.rs:296-334) over ONE committee and a participation bitmap per instance (blsw_committee_verify_batch,
    // include/blsw.h): bitmaps[i][k] != 0 selects committee[k] for instance i. group == 0: one verdict per instance — true iff the selection is not
    // empty, every selected key decodes, the sum is not the identity and BLS::verify accepts it. group >= 1: one verdict per group of instances,
    // verify_groups' statement over the aggregated keys; scalars as there (empty draws group_scalars(n); ignored for group == 0).
    // status [n][2] (aggregate key, signature), key_status [K], counts [n], aggregates [n] (the compressed sums) are filled when given.
    static std::vector<bool> fast_aggregate_verify_committee(const Parameters&, const std::vector<PublicKey>& committee, const std::vector<std::vector<uint8_t>>& bitmaps,
                                                             const std::vector<std::vector<uint8_t>>& messages, const std::vector<Signature>& sigs, uint32_t group = 0,
                                                             std::vector<uint64_t> scalars = {}, std::vector<int32_t>* status = nullptr,
                                                             std::vector<int32_t>* key_status = nullptr, std::vector<uint32_t>* counts = nullptr,
                                                             std::vector<PublicKey>* aggregates = nullptr, const Dst& dst = Dst()) {
        const size_t n = bitmaps.size(), K = committee.size();
        if (n == 0 || K == 0 || K > 65535 || messages.size() != n || sigs.size() != n)
            throw Error("BLS::fast_aggregate_verify_committee: a committee, and one bitmap, message and signature per instance", BLSW_ERR_ARG);
        if (group) {
            if (scalars.empty()) scalars = group_scalars(n);
            if (scalars.size() != n) throw Error("BLS::fast_aggregate_verify_committee: one coefficient per instance", BLSW_ERR_ARG);
        }
        const uint32_t msg_len = (uint32_t)messages[0].size();
        std::vector<uint8_t> pk(K * 48), bm(n * K), sg(n * 96), msg(n * (size_t)msg_len);
        for (size_t k = 0; k < K; k++) std::memcpy(&pk[48 * k], committee[k].bytes.data(), 48);
        for (size_t i = 0; i < n; i++) {
            if (messages[i].size() != msg_len) throw Error("BLS::fast_aggregate_verify_committee: messages of one length per batch", BLSW_ERR_ARG);
            if (bitmaps[i].size() != K) throw Error("BLS::fast_aggregate_verify_committee: one bitmap byte per committee key", BLSW_ERR_ARG);
            std::memcpy(&bm[K * i], bitmaps[i].data(), K);
            std::memcpy(&sg[96 * i], sigs[i].bytes.data(), 96);
            if (msg_len) std::memcpy(&msg[(size_t)msg_len * i], messages[i].data(), msg_len);
        }
        const size_t n_res = group ? (n + group - 1) / group : n;
        uint64_t bytes = 0;
        check(blsw_committee_verify_workspace_bytes(n, msg_len, (uint32_t)K, group, &bytes), "blsw_committee_verify_workspace_bytes");
        detail::DeviceBytes ws(bytes), d_pk(pk.size()), d_bm(bm.size()), d_sg(sg.size()), d_msg(msg.size()), d_sc(n * 8), d_st(n * 8), d_kst(K * 4), d_cnt(n * 4), d_agg(n * 48),
            d_res(n_res * 4);
        d_pk.upload(pk.data(), pk.size());
        d_bm.upload(bm.data(), bm.size());
        d_sg.upload(sg.data(), sg.size());
        if (group) d_sc.upload(scalars.data(), n * 8);
        if (!msg.empty()) d_msg.upload(msg.data(), msg.size());
        check(blsw_committee_verify_batch_dst(static_cast<const uint8_t*>(d_pk.get()), (uint32_t)K, static_cast<const uint8_t*>(d_bm.get()), static_cast<const uint8_t*>(d_sg.get()),
                                          static_cast<const uint8_t*>(d_msg.get()), msg_len, n, group ? static_cast<const uint64_t*>(d_sc.get()) : nullptr, group,
                                          static_cast<int32_t*>(d_res.get()), static_cast<uint32_t*>(d_cnt.get()), static_cast<int32_t*>(d_st.get()),
                                          static_cast<int32_t*>(d_kst.get()), static_cast<uint8_t*>(d_agg.get()), ws.get(), bytes, dst.get(), nullptr),
              "blsw_committee_verify_batch");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        std::vector<int32_t> r(n_res);
        d_res.download(r.data(), n_res * 4);
        if (status) {
            status->resize(2 * n);
            d_st.download(status->data(), n * 8);
        }
        if (key_status) {
            key_status->resize(K);
            d_kst.download(key_status->data(), K * 4);
        }
        if (counts) {
            counts->resize(n);
            d_cnt.download(counts->data(), n * 4);
        }
        if (aggregates) {
            std::vector<uint8_t> a(n * 48);
            d_agg.download(a.data(), a.size());
            aggregates->resize(n);
            for (size_t i = 0; i < n; i++) std::memcpy((*aggregates)[i].bytes.data(), &a[48 * i], 48);
        }
        std::vector<bool> out(n_res);
        for (size_t j = 0; j < n_res; j++) out[j] = r[j] == 1;
        return out;
    }
    // the per-instance verdicts through groups: the instances of passing groups are true, those of failing groups go through the per-instance form
    // once more (the committee is decoded again: K lanes). Slower than group == 0 when most groups hold a bad instance.
    static std::vector<bool> fast_aggregate_verify_committee_grouped(const Parameters& params, const std::vector<PublicKey>& committee,
                                                                     const std::vector<std::vector<uint8_t>>& bitmaps, const std::vector<std::vector<uint8_t>>& messages,
                                                                     const std::vector<Signature>& sigs, uint32_t group = 64, std::vector<uint64_t> scalars = {},
                                                                     std::vector<int32_t>* status = nullptr, const Dst& dst = Dst()) {
        if (group == 0) throw Error("BLS::fast_aggregate_verify_committee_grouped: group >= 1", BLSW_ERR_ARG);
        const std::vector<bool> g = fast_aggregate_verify_committee(params, committee, bitmaps, messages, sigs, group, std::move(scalars), status, nullptr, nullptr, nullptr, dst);
        const size_t n = bitmaps.size();
        std::vector<bool> out(n, true);
        std::vector<size_t> idx;
        for (size_t i = 0; i < n; i++)
            if (!g[i / group]) idx.push_back(i);
        if (idx.empty()) return out;
        std::vector<std::vector<uint8_t>> b2, m2;
        std::vector<Signature> s2;
        for (size_t i : idx) {
            b2.push_back(bitmaps[i]);
            m2.push_back(messages[i]);
            s2.push_back(sigs[i]);
        }
        const std::vector<bool> r = fast_aggregate_verify_committee(params, committee, b2, m2, s2, 0, {}, nullptr, nullptr, nullptr, nullptr, dst);
        for (size_t k = 0; k < idx.size(); k++) out[idx[k]] = r[k];
        return out;
    }
    // fast_aggregate_verify over a resident KeyRegistry and one list of key INDICES per set (blsw_registry_verify_batch, include/blsw.h): a repeated
    // index is added as often as it occurs. group == 0: one verdict per set — true iff the list is not empty, every index is below registry.size(),
    // every named key decodes, the sum is not the identity and BLS::verify accepts it. group >= 1: one verdict per group of sets, verify_groups'
    // statement over the sums; scalars as there (empty draws group_scalars(n); ignored for group == 0).
    // status [n][2] (the set's key — BLSW_ST_BAD_INDEX for an index >= size —, signature) and aggregates [n] (the compressed sums) are filled when given.
    static std::vector<bool> fast_aggregate_verify_indexed(const Parameters&, const KeyRegistry& registry, const std::vector<std::vector<uint32_t>>& index_lists,
                                                           const std::vector<std::vector<uint8_t>>& messages, const std::vector<Signature>& sigs, uint32_t group = 0,
                                                           std::vector<uint64_t> scalars = {}, std::vector<int32_t>* status = nullptr,
                                                           std::vector<PublicKey>* aggregates = nullptr, const Dst& dst = Dst()) {
        const size_t n = index_lists.size();
        if (n == 0 || messages.size() != n || sigs.size() != n)
            throw Error("BLS::fast_aggregate_verify_indexed: one index list, message and signature per set", BLSW_ERR_ARG);
        if (group) {
            if (scalars.empty()) scalars = group_scalars(n);
            if (scalars.size() != n) throw Error("BLS::fast_aggregate_verify_indexed: one coefficient per set", BLSW_ERR_ARG);
        }
        const uint32_t msg_len = (uint32_t)messages[0].size();
        std::vector<uint64_t> off(n + 1, 0);
        for (size_t i = 0; i < n; i++) off[i + 1] = off[i] + index_lists[i].size();
        std::vector<uint32_t> idx(off[n]);
        std::vector<uint8_t> sg(n * 96), msg(n * (size_t)msg_len);
        for (size_t i = 0; i < n; i++) {
            if (messages[i].size() != msg_len) throw Error("BLS::fast_aggregate_verify_indexed: messages of one length per batch", BLSW_ERR_ARG);
            if (!index_lists[i].empty()) std::memcpy(&idx[off[i]], index_lists[i].data(), index_lists[i].size() * 4);
            std::memcpy(&sg[96 * i], sigs[i].bytes.data(), 96);
            if (msg_len) std::memcpy(&msg[(size_t)msg_len * i], messages[i].data(), msg_len);
        }
        const size_t n_res = group ? (n + group - 1) / group : n;
        uint64_t bytes = 0;
        check(blsw_registry_verify_workspace_bytes(n, msg_len, group, &bytes), "blsw_registry_verify_workspace_bytes");
        detail::DeviceBytes ws(bytes), d_idx(idx.size() * 4), d_off(off.size() * 8), d_sg(sg.size()), d_msg(msg.size()), d_sc(n * 8), d_st(n * 8), d_agg(n * 48), d_res(n_res * 4);
        if (!idx.empty()) d_idx.upload(idx.data(), idx.size() * 4);
        d_off.upload(off.data(), off.size() * 8);
        d_sg.upload(sg.data(), sg.size());
        if (group) d_sc.upload(scalars.data(), n * 8);
        if (!msg.empty()) d_msg.upload(msg.data(), msg.size());
        check(blsw_registry_verify_batch_dst(registry.get(), idx.empty() ? nullptr : static_cast<const uint32_t*>(d_idx.get()), idx.size(), static_cast<const uint64_t*>(d_off.get()),
                                         static_cast<const uint8_t*>(d_sg.get()), static_cast<const uint8_t*>(d_msg.get()), msg_len, n,
                                         group ? static_cast<const uint64_t*>(d_sc.get()) : nullptr, group, static_cast<int32_t*>(d_res.get()), static_cast<int32_t*>(d_st.get()),
                                         static_cast<uint8_t*>(d_agg.get()), ws.get(), bytes, dst.get(), nullptr),
              "blsw_registry_verify_batch");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        std::vector<int32_t> r(n_res);
        d_res.download(r.data(), n_res * 4);
        if (status) {
            status->resize(2 * n);
            d_st.download(status->data(), n * 8);
        }
        if (aggregates) {
            std::vector<uint8_t> a(n * 48);
            d_agg.download(a.data(), a.size());
            aggregates->resize(n);
            for (size_t i = 0; i < n; i++) std::memcpy((*aggregates)[i].bytes.data(), &a[48 * i], 48);
        }
        std::vector<bool> out(n_res);
        for (size_t j = 0; j < n_res; j++) out[j] = r[j] == 1;
        return out;
    }
    // fast_aggregate_verify_indexed (group >= 1) over a message TABLE (blsw_registry_verify_shared_batch, include/blsw.h): set i signs
    // table[msg_index[i]]; one hash per table row, one pair per run of equal adjacent indices of a group — sort each group by index. An index beyond
    // the table is BLSW_ST_BAD_INDEX in status[2 i], in front of the registry's own rules. runs (when given) receives the runs of each group.
    static std::vector<bool> fast_aggregate_verify_indexed_shared(const Parameters&, const KeyRegistry& registry, const std::vector<std::vector<uint32_t>>& index_lists,
                                                                  const std::vector<std::vector<uint8_t>>& table, const std::vector<uint32_t>& msg_index,
                                                                  const std::vector<Signature>& sigs, uint32_t group = 64, std::vector<uint64_t> scalars = {},
                                                                  std::vector<int32_t>* status = nullptr, std::vector<PublicKey>* aggregates = nullptr,
                                                                  std::vector<uint32_t>* runs = nullptr, const Dst& dst = Dst()) {
        const size_t n = index_lists.size(), n_msgs = table.size();
        if (n == 0 || n_msgs == 0 || msg_index.size() != n || sigs.size() != n || group == 0)
            throw Error("BLS::fast_aggregate_verify_indexed_shared: a table, and one index list, message index and signature per set", BLSW_ERR_ARG);
        if (scalars.empty()) scalars = group_scalars(n);
        if (scalars.size() != n) throw Error("BLS::fast_aggregate_verify_indexed_shared: one coefficient per set", BLSW_ERR_ARG);
        const uint32_t msg_len = (uint32_t)table[0].size();
        std::vector<uint64_t> off(n + 1, 0);
        for (size_t i = 0; i < n; i++) off[i + 1] = off[i] + index_lists[i].size();
        std::vector<uint32_t> idx(off[n]);
        std::vector<uint8_t> sg(n * 96), msg(n_msgs * (size_t)msg_len);
        for (size_t i = 0; i < n; i++) {
            if (!index_lists[i].empty()) std::memcpy(&idx[off[i]], index_lists[i].data(), index_lists[i].size() * 4);
            std::memcpy(&sg[96 * i], sigs[i].bytes.data(), 96);
        }
        for (size_t r = 0; r < n_msgs; r++) {
            if (table[r].size() != msg_len) throw Error("BLS::fast_aggregate_verify_indexed_shared: messages of one length per table", BLSW_ERR_ARG);
            if (msg_len) std::memcpy(&msg[(size_t)msg_len * r], table[r].data(), msg_len);
        }
        const size_t n_groups = (n + group - 1) / group;
        uint64_t bytes = 0;
        check(blsw_registry_verify_shared_workspace_bytes(n, n_msgs, msg_len, group, &bytes), "blsw_registry_verify_shared_workspace_bytes");
        detail::DeviceBytes ws(bytes), d_idx(idx.size() * 4), d_off(off.size() * 8), d_sg(sg.size()), d_msg(msg.size()), d_ix(n * 4), d_sc(n * 8), d_st(n * 8), d_agg(n * 48),
            d_res(n_groups * 4), d_runs(n_groups * 4);
        if (!idx.empty()) d_idx.upload(idx.data(), idx.size() * 4);
        d_off.upload(off.data(), off.size() * 8);
        d_sg.upload(sg.data(), sg.size());
        d_ix.upload(msg_index.data(), n * 4);
        d_sc.upload(scalars.data(), n * 8);
        if (!msg.empty()) d_msg.upload(msg.data(), msg.size());
        check(blsw_registry_verify_shared_batch(registry.get(), idx.empty() ? nullptr : static_cast<const uint32_t*>(d_idx.get()), idx.size(), static_cast<const uint64_t*>(d_off.get()),
                                                static_cast<const uint8_t*>(d_sg.get()), static_cast<const uint8_t*>(d_msg.get()), msg_len, n_msgs,
                                                static_cast<const uint32_t*>(d_ix.get()), n, static_cast<const uint64_t*>(d_sc.get()), group, dst.get(),
                                                static_cast<int32_t*>(d_res.get()), static_cast<uint32_t*>(d_runs.get()), static_cast<int32_t*>(d_st.get()),
                                                static_cast<uint8_t*>(d_agg.get()), ws.get(), bytes, nullptr),
              "blsw_registry_verify_shared_batch");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        std::vector<int32_t> r(n_groups);
        d_res.download(r.data(), n_groups * 4);
        if (status) {
            status->resize(2 * n);
            d_st.download(status->data(), n * 8);
        }
        if (aggregates) {
            std::vector<uint8_t> a(n * 48);
            d_agg.download(a.data(), a.size());
            aggregates->resize(n);
            for (size_t i = 0; i < n; i++) std::memcpy((*aggregates)[i].bytes.data(), &a[48 * i], 48);
        }
        if (runs) {
            runs->resize(n_groups);
            d_runs.download(runs->data(), n_groups * 4);
        }
        std::vector<bool> out(n_groups);
        for (size_t j = 0; j < n_groups; j++) out[j] = r[j] == 1;
        return out;
    }
    // the per-set verdicts through groups: the sets of passing groups are true, those of failing groups go through the per-set form once more (the
    // registry is not decoded again: it is resident). Slower than group == 0 when most groups hold a bad set.
    static std::vector<bool> fast_aggregate_verify_indexed_grouped(const Parameters& params, const KeyRegistry& registry, const std::vector<std::vector<uint32_t>>& index_lists,
                                                                   const std::vector<std::vector<uint8_t>>& messages, const std::vector<Signature>& sigs, uint32_t group = 64,
                                                                   std::vector<uint64_t> scalars = {}, std::vector<int32_t>* status = nullptr, const Dst& dst = Dst()) {
        if (group == 0) throw Error("BLS::fast_aggregate_verify_indexed_grouped: group >= 1", BLSW_ERR_ARG);
        const std::vector<bool> g = fast_aggregate_verify_indexed(params, registry, index_lists, messages, sigs, group, std::move(scalars), status, nullptr, dst);
        const size_t n = index_lists.size();
        std::vector<bool> out(n, true);
        std::vector<size_t> idx;
        for (size_t i = 0; i < n; i++)
            if (!g[i / group]) idx.push_back(i);
        if (idx.empty()) return out;
        std::vector<std::vector<uint32_t>> l2;
        std::vector<std::vector<uint8_t>> m2;
        std::vector<Signature> s2;
        for (size_t i : idx) {
            l2.push_back(index_lists[i]);
            m2.push_back(messages[i]);
            s2.push_back(sigs[i]);
        }
        const std::vector<bool> r = fast_aggregate_verify_indexed(params, registry, l2, m2, s2, 0, {}, nullptr, nullptr, dst);
        for (size_t k = 0; k < idx.size(); k++) out[idx[k]] = r[k];
        return out;
    }
    // AggregateVerify of the signature draft as values (blsw_verify_pairs_batch, include/blsw.h): instance i is ONE aggregate signature over the pairs
    // (key_lists[i][j], message_lists[i][j]) with their own messages. The lists may be ragged: they travel padded to the longest with their counts.
    // True iff the list is not empty, every key decodes to a non-identity point of the subgroup (an identity key is refused, unlike a summand of
    // fast_aggregate_verify), the signature decodes and e(-g1, sig) * prod_j e(pk_j, H(m_j)) == 1. All messages of a batch have one length.
    // status [n][2] (the instance's keys and count, the signature) and key_status [n][longest] (every key, the padding included) are filled when given.
    static std::vector<bool> aggregate_verify(const Parameters&, const std::vector<std::vector<PublicKey>>& key_lists,
                                              const std::vector<std::vector<std::vector<uint8_t>>>& message_lists, const std::vector<Signature>& sigs,
                                              std::vector<int32_t>* status = nullptr, std::vector<int32_t>* key_status = nullptr, const Dst& dst = Dst()) {
        const size_t n = key_lists.size();
        if (n == 0 || message_lists.size() != n || sigs.size() != n) throw Error("BLS::aggregate_verify: one key list, message list and signature per instance", BLSW_ERR_ARG);
        size_t K = 1, msg_len = 0;
        bool have_len = false;
        for (size_t i = 0; i < n; i++) {
            if (message_lists[i].size() != key_lists[i].size()) throw Error("BLS::aggregate_verify: one message per key", BLSW_ERR_ARG);
            K = std::max(K, key_lists[i].size());
            for (const std::vector<uint8_t>& m : message_lists[i]) {
                if (have_len && m.size() != msg_len) throw Error("BLS::aggregate_verify: messages of one length per batch", BLSW_ERR_ARG);
                msg_len = m.size();
                have_len = true;
            }
        }
        if (K > 65535) throw Error("BLS::aggregate_verify: at most 65535 pairs per instance", BLSW_ERR_ARG);
        std::vector<uint8_t> pk(n * K * 48, 0), msg(n * K * msg_len, 0), sg(n * 96);
        std::vector<uint32_t> counts(n);
        for (size_t i = 0; i < n; i++) {
            counts[i] = (uint32_t)key_lists[i].size();
            for (size_t j = 0; j < key_lists[i].size(); j++) {
                std::memcpy(&pk[48 * (i * K + j)], key_lists[i][j].bytes.data(), 48);
                if (msg_len) std::memcpy(&msg[msg_len * (i * K + j)], message_lists[i][j].data(), msg_len);
            }
            std::memcpy(&sg[96 * i], sigs[i].bytes.data(), 96);
        }
        uint64_t bytes = 0;
        check(blsw_verify_pairs_workspace_bytes(n, (uint32_t)msg_len, (uint32_t)K, &bytes), "blsw_verify_pairs_workspace_bytes");
        detail::DeviceBytes ws(bytes), d_pk(pk.size()), d_msg(msg.size()), d_sg(sg.size()), d_cnt(n * 4), d_st(n * 8), d_kst(n * K * 4), d_res(n * 4);
        d_pk.upload(pk.data(), pk.size());
        if (!msg.empty()) d_msg.upload(msg.data(), msg.size());
        d_sg.upload(sg.data(), sg.size());
        d_cnt.upload(counts.data(), n * 4);
        check(blsw_verify_pairs_batch_dst(static_cast<const uint8_t*>(d_pk.get()), static_cast<const uint8_t*>(d_msg.get()), (uint32_t)msg_len, (uint32_t)K,
                                      static_cast<const uint32_t*>(d_cnt.get()), static_cast<const uint8_t*>(d_sg.get()), n, static_cast<int32_t*>(d_res.get()),
                                      static_cast<int32_t*>(d_st.get()), static_cast<int32_t*>(d_kst.get()), ws.get(), bytes, dst.get(), nullptr),
              "blsw_verify_pairs_batch");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        std::vector<int32_t> r(n);
        d_res.download(r.data(), n * 4);
        if (status) {
            status->resize(2 * n);
            d_st.download(status->data(), n * 8);
        }
        if (key_status) {
            key_status->resize(n * K);
            d_kst.download(key_status->data(), n * K * 4);
        }
        std::vector<bool> out(n);
        for (size_t i = 0; i < n; i++) out[i] = r[i] == 1;
        return out;
    }
    // PopProve of the signature draft's POP ciphersuite (blsw_pop_prove_batch): the keys and, per key, proof = sk * hash_to_g2(pk's 48 bytes, Dst::pop()).
    struct Proved {
        std::vector<PublicKey> public_keys;
        std::vector<Signature> proofs;   // the infinity encoding where status != BLSW_ST_OK
        std::vector<int32_t> status;     // as Signed::status
    };
    static Proved pop_prove(const Parameters&, const std::vector<SecretKey>& sks) {
        const size_t n = sks.size();
        if (n == 0) throw Error("BLS::pop_prove: at least one key", BLSW_ERR_ARG);
        std::vector<uint8_t> sk(n * 32);
        for (size_t i = 0; i < n; i++) std::memcpy(&sk[32 * i], sks[i].le.data(), 32);
        uint64_t bytes = 0;
        check(blsw_hash_to_g2_workspace_bytes(n, 48, &bytes), "blsw_hash_to_g2_workspace_bytes");
        detail::DeviceBytes d_sk(sk.size()), d_proof(n * 96), d_pk(n * 48), d_st(n * 4), ws(bytes);
        d_sk.upload(sk.data(), sk.size());
        check(blsw_pop_prove_batch(static_cast<const uint8_t*>(d_sk.get()), n, static_cast<uint8_t*>(d_proof.get()), static_cast<uint8_t*>(d_pk.get()),
                                   static_cast<int32_t*>(d_st.get()), ws.get(), bytes, nullptr),
              "blsw_pop_prove_batch");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        std::vector<uint8_t> pr(n * 96), pk(n * 48);
        Proved out;
        out.status.resize(n);
        d_proof.download(pr.data(), pr.size());
        d_pk.download(pk.data(), pk.size());
        d_st.download(out.status.data(), n * 4);
        out.proofs.resize(n);
        out.public_keys.resize(n);
        for (size_t i = 0; i < n; i++) {
            std::memcpy(out.proofs[i].bytes.data(), &pr[96 * i], 96);
            std::memcpy(out.public_keys[i].bytes.data(), &pk[48 * i], 48);
        }
        return out;
    }
    // PopVerify (blsw_pop_verify_batch): KeyValidate and the pairing check of the proof over the key's own bytes under Dst::pop(); status [n][2] (key, proof)
    static std::vector<bool> pop_verify(const Parameters&, const std::vector<PublicKey>& pks, const std::vector<Signature>& proofs, std::vector<int32_t>* status = nullptr) {
        const size_t n = pks.size();
        if (n == 0 || proofs.size() != n) throw Error("BLS::pop_verify: one proof per key", BLSW_ERR_ARG);
        std::vector<uint8_t> pk(n * 48), pr(n * 96);
        for (size_t i = 0; i < n; i++) {
            std::memcpy(&pk[48 * i], pks[i].bytes.data(), 48);
            std::memcpy(&pr[96 * i], proofs[i].bytes.data(), 96);
        }
        uint64_t bytes = 0;
        check(blsw_verify_workspace_bytes(n, 48, &bytes), "blsw_verify_workspace_bytes");
        detail::DeviceBytes ws(bytes), d_pk(pk.size()), d_pr(pr.size()), d_st(n * 8), d_res(n * 4);
        d_pk.upload(pk.data(), pk.size());
        d_pr.upload(pr.data(), pr.size());
        check(blsw_pop_verify_batch(static_cast<const uint8_t*>(d_pk.get()), static_cast<const uint8_t*>(d_pr.get()), n, static_cast<int32_t*>(d_res.get()),
                                    static_cast<int32_t*>(d_st.get()), ws.get(), bytes, nullptr),
              "blsw_pop_verify_batch");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        std::vector<int32_t> r(n);
        d_res.download(r.data(), n * 4);
        if (status) {
            status->resize(2 * n);
            d_st.download(status->data(), n * 8);
        }
        std::vector<bool> out(n);
        for (size_t i = 0; i < n; i++) out[i] = r[i] == 1;
        return out;
    }
    // Weighted point sums and threshold recovery (blsw_combine_points_batch, blsw_lagrange_batch, blsw_recover_points_batch): one list per entry of
    // the outer vector, lists of different lengths travel padded to the longest with their counts. A Scalar is 32 little-endian bytes of an element
    // of Fr, and PUBLIC: the ladders are not constant-time. status (optional) [n] as the header states it; a failing list gives an all-zero point.
    using Scalar = std::array<uint8_t, 32>;
    static std::vector<Signature> combine(const std::vector<std::vector<Signature>>& points, const std::vector<std::vector<Scalar>>& scalars, std::vector<int32_t>* status = nullptr) {
        return combine_lists<Signature>(2, points, scalars, Sum::Ladders, status);
    }
    static std::vector<PublicKey> combine(const std::vector<std::vector<PublicKey>>& points, const std::vector<std::vector<Scalar>>& scalars, std::vector<int32_t>* status = nullptr) {
        return combine_lists<PublicKey>(1, points, scalars, Sum::Ladders, status);
    }
    // The same sums by the bucket method (blsw_msm_points_batch): lists of up to 2^24 terms; window_bits 0 is the library's choice. For every input
    // combine accepts the points and statuses are the same bytes; the header says which of the two suits which shape.
    static std::vector<Signature> msm(const std::vector<std::vector<Signature>>& points, const std::vector<std::vector<Scalar>>& scalars, std::vector<int32_t>* status = nullptr,
                                      uint32_t window_bits = 0) {
        return combine_lists<Signature>(2, points, scalars, Sum::Buckets, status, window_bits);
    }
    static std::vector<PublicKey> msm(const std::vector<std::vector<PublicKey>>& points, const std::vector<std::vector<Scalar>>& scalars, std::vector<int32_t>* status = nullptr,
                                      uint32_t window_bits = 0) {
        return combine_lists<PublicKey>(1, points, scalars, Sum::Buckets, status, window_bits);
    }
    // the group signature / group key from the shares' partial signatures / keys at the shares' ids (Lagrange interpolation at 0 in the exponent)
    static std::vector<Signature> recover_signature(const std::vector<std::vector<Scalar>>& ids, const std::vector<std::vector<Signature>>& sigs, std::vector<int32_t>* status = nullptr) {
        return combine_lists<Signature>(2, sigs, ids, Sum::Recover, status);
    }
    static std::vector<PublicKey> recover_public_key(const std::vector<std::vector<Scalar>>& ids, const std::vector<std::vector<PublicKey>>& pks, std::vector<int32_t>* status = nullptr) {
        return combine_lists<PublicKey>(1, pks, ids, Sum::Recover, status);
    }
    // lambda_j = prod_{m != j} id_m / prod_{m != j} (id_m - id_j) per list; an empty inner vector where the list fails (status says why)
    static std::vector<std::vector<Scalar>> lagrange_coefficients(const std::vector<std::vector<Scalar>>& ids, std::vector<int32_t>* status = nullptr) {
        const size_t n = ids.size();
        std::vector<uint32_t> counts;
        const uint32_t k = pad_counts(ids, counts, "BLS::lagrange_coefficients");
        std::vector<uint8_t> rows = pad_rows(ids, k);
        detail::DeviceBytes d_ids(rows.size()), d_cnt(n * 4), d_coeff(rows.size()), d_st(n * 4);
        d_ids.upload(rows.data(), rows.size());
        d_cnt.upload(counts.data(), n * 4);
        check(blsw_lagrange_batch(static_cast<const uint8_t*>(d_ids.get()), static_cast<const uint32_t*>(d_cnt.get()), k, n, static_cast<uint8_t*>(d_coeff.get()),
                                  static_cast<int32_t*>(d_st.get()), nullptr),
              "blsw_lagrange_batch");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        std::vector<int32_t> st(n);
        d_coeff.download(rows.data(), rows.size());
        d_st.download(st.data(), n * 4);
        std::vector<std::vector<Scalar>> out(n);
        for (size_t i = 0; i < n; i++) {
            if (st[i] != BLSW_ST_OK) continue;
            out[i].resize(counts[i]);
            for (size_t j = 0; j < counts[i]; j++) std::memcpy(out[i][j].data(), &rows[(i * k + j) * 32], 32);
        }
        if (status) *status = st;
        return out;
    }

   private:
    template <class LISTS>
    static uint32_t pad_counts(const LISTS& lists, std::vector<uint32_t>& counts, const char* who, size_t max_k = 65535) {
        size_t k = 0;
        for (const auto& l : lists) k = std::max(k, l.size());
        if (lists.empty() || k == 0 || k > max_k) throw Error(std::string(who) + ": at least one list, 1 .. " + std::to_string(max_k) + " terms in the longest", BLSW_ERR_ARG);
        counts.resize(lists.size());
        for (size_t i = 0; i < lists.size(); i++) counts[i] = static_cast<uint32_t>(lists[i].size());
        return static_cast<uint32_t>(k);
    }
    static std::vector<uint8_t> pad_rows(const std::vector<std::vector<Scalar>>& lists, uint32_t k) {
        std::vector<uint8_t> rows(lists.size() * k * 32, 0);
        for (size_t i = 0; i < lists.size(); i++)
            for (size_t j = 0; j < lists[i].size(); j++) std::memcpy(&rows[(i * k + j) * 32], lists[i][j].data(), 32);
        return rows;
    }
    // which C entry forms the sums: blsw_combine_points_batch, blsw_recover_points_batch, blsw_msm_points_batch (the only one that reads window_bits)
    enum class Sum { Ladders, Recover, Buckets };
    template <class POINT>
    static std::vector<POINT> combine_lists(uint32_t group, const std::vector<std::vector<POINT>>& points, const std::vector<std::vector<Scalar>>& rows32, Sum how,
                                            std::vector<int32_t>* status, uint32_t window_bits = 0) {
        const size_t n = points.size(), W = sizeof(POINT::bytes);
        const bool msm = how == Sum::Buckets, recover = how == Sum::Recover;
        const char* who = recover ? "BLS::recover" : msm ? "BLS::msm" : "BLS::combine";
        if (rows32.size() != n) throw Error(std::string(who) + ": one list of scalars or ids per list of points", BLSW_ERR_ARG);
        for (size_t i = 0; i < n; i++)
            if (rows32[i].size() != points[i].size()) throw Error(std::string(who) + ": one scalar or id per point", BLSW_ERR_ARG);
        std::vector<uint32_t> counts;
        const uint32_t k = pad_counts(points, counts, who, msm ? size_t(1) << 24 : 65535);
        std::vector<uint8_t> in(n * k * W, 0), rows = pad_rows(rows32, k);
        for (size_t i = 0; i < n; i++)
            for (size_t j = 0; j < points[i].size(); j++) std::memcpy(&in[(i * k + j) * W], points[i][j].bytes.data(), W);
        uint64_t bytes = 0;
        if (msm)
            check(blsw_msm_workspace_bytes(group, n, k, window_bits, &bytes), "blsw_msm_workspace_bytes");
        else
            check(blsw_combine_points_workspace_bytes(group, n, k, &bytes), "blsw_combine_points_workspace_bytes");
        detail::DeviceBytes d_in(in.size()), d_rows(rows.size()), d_cnt(n * 4), d_out(n * W), d_st(n * 4), ws(bytes);
        d_in.upload(in.data(), in.size());
        d_rows.upload(rows.data(), rows.size());
        d_cnt.upload(counts.data(), n * 4);
        const uint8_t *p_in = static_cast<const uint8_t*>(d_in.get()), *p_rows = static_cast<const uint8_t*>(d_rows.get());
        const uint32_t* p_cnt = static_cast<const uint32_t*>(d_cnt.get());
        if (recover)
            check(blsw_recover_points_batch(group, p_in, p_rows, p_cnt, k, n, static_cast<uint8_t*>(d_out.get()), static_cast<int32_t*>(d_st.get()), ws.get(), bytes, nullptr),
                  "blsw_recover_points_batch");
        else if (msm)
            check(blsw_msm_points_batch(group, p_in, p_rows, p_cnt, k, n, window_bits, static_cast<uint8_t*>(d_out.get()), static_cast<int32_t*>(d_st.get()), ws.get(),
                                        bytes, nullptr),
                  "blsw_msm_points_batch");
        else
            check(blsw_combine_points_batch(group, p_in, p_rows, p_cnt, k, n, static_cast<uint8_t*>(d_out.get()), static_cast<int32_t*>(d_st.get()), nullptr, ws.get(), bytes, nullptr),
                  "blsw_combine_points_batch");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        std::vector<uint8_t> o(n * W);
        d_out.download(o.data(), o.size());
        if (status) {
            status->resize(n);
            d_st.download(status->data(), n * 4);
        }
        std::vector<POINT> out(n);
        for (size_t i = 0; i < n; i++) std::memcpy(out[i].bytes.data(), &o[W * i], W);
        return out;
    }
};

}  // namespace blsw
