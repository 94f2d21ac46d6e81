/* blsw — MI355X-native batched witness generation for the BLS12-381 signature-verify R1CS gadget.
 *
 * C ABI of libblsw.so (HIP, gfx950). The reference (lightec-xyz/bls-verify-gadget) has NO FFI: the path sits
 * behind the arkworks trait surface
 *     impl SigVerifyGadget<BLS<P>, P::Fp> for BlsSignatureVerifyGadget<P>::verify     src/constraints.rs:79-128
 *     AllocVar for ParametersVar / PublicKeyVar / SignatureVar                         src/constraints.rs:194-249
 *     hash_to_g2_with_cons(cs, &[UInt8]) -> G2Var                                      src/hasher.rs:727-740
 * and the data an arkworks prover consumes from it is ConstraintSystem::witness_assignment (Vec<Fq>, Montgomery
 * form, allocation order) plus the constraint matrices of cs.to_matrices(). These entry points replace exactly that
 * side effect, batched over instances; they are what a Rust `extern "C"` shim binds.
 * tests/test_abi_contract.py parses THIS file and fails when INTEGRATION.md's Rust block, the ctypes binding or the
 * library's exports drift from it.
 *
 * Conventions: caller-allocated buffers, integer return codes (0 = ok), no exceptions across the ABI,
 * re-entrant per (device, stream). All `d_*` pointers are DEVICE pointers on the engine's / current HIP device.
 * A field element is 6 little-endian u64 limbs in Montgomery form (R = 2^384) == arkworks' in-memory Fq.
 */
#ifndef BLSW_H
#define BLSW_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define BLSW_ABI_VERSION 17

#define BLSW_OK 0
#define BLSW_ERR_ARG 1
#define BLSW_ERR_WORKSPACE 2
#define BLSW_ERR_HIP 3
#define BLSW_ERR_NO_DEVICE 4
#define BLSW_ERR_SCRATCH 5 /* the requested mode / n_buffers combination would exhaust the runtime's per-queue scratch */
#define BLSW_ERR_BUSY 6    /* consumer mode: the call has to wait for outputs the caller still holds (drain and release first) */

/* per-instance input status (mirrors src/bls.rs:434-447 and the deserialization fixtures) */
#define BLSW_ST_OK 0
#define BLSW_ST_BAD_ENCODING 1
#define BLSW_ST_NOT_ON_CURVE 2
#define BLSW_ST_NOT_IN_SUBGROUP 3
#define BLSW_ST_IDENTITY 4
#define BLSW_ST_INVALID_SECRET_KEY 5
#define BLSW_ST_BAD_INDEX 6 /* blsw_registry_verify_batch: offsets that describe no list, or an index at or beyond the registry's size */
#define BLSW_ST_BAD_ID 7    /* blsw_lagrange_batch / blsw_recover_points_batch: a used id that is zero or equal to another used id of its list */

/* Segment table of one instance's witness vector for the circuit of src/constraints.rs:335-366
 * (msg witness bytes, params Constant, pk Witness, sig Witness, then verify). Offsets are in field elements.
 * 36 uint32_t fields; the Rust mirror in INTEGRATION.md must have the same fields in the same order. */
typedef struct {
    uint32_t msg_len;
    uint32_t n_instance_vars; /* instance_assignment length: 1 (the constant one) + c message chunks if the message is Input (blsw_layout_inputs)
                               * + 3 if pk_mode is Input + 6 if sig_mode is Input */
    uint32_t n_witness;       /* witness_assignment length */
    uint32_t sha_bits;        /* boolean witnesses of ONE expand_message segment (16 lib_str bits + SHA-256 gadget) */
    uint32_t off_msg, off_pk_alloc, off_sig_alloc, off_pk_not_zero, off_expand, off_map0, off_map1, off_add, off_cofactor, off_prep_h, off_prep_pk,
        off_prep_sig, off_miller, off_final_exp, off_is_one;
    /* aggregate_verify circuits (src/constraints.rs:378-441); all zero for the single-key circuit (then off_pk_alloc is used) */
    uint32_t n_keys, off_keys, off_bitmap, off_count, off_agg;
    /* N+1-pair product (blsw_layout_multi): the segments msg, pk_alloc, pk_not_zero, {expand, map0, map1, add, cofactor},
     * prep_h and prep_pk exist once per (pk, msg) pair; pair j's copy starts at off_* + j * stride_*. n_pairs = 1 and
     * strides = segment lengths for the single-key and aggregate circuits. */
    uint32_t n_pairs, stride_msg, stride_pk_alloc, stride_pk_not_zero, stride_hash, stride_prep_h, stride_prep_pk;
    /* ParametersVar allocated with AllocationMode::Witness (blsw_layout_params; src/constraints.rs:198-211 takes any mode): the
     * generator's G1Var::new_variable segment between msg and pk_alloc, and prepare_g1(-g1) (to_affine, 7 witnesses) in front of
     * prep_h; the ell of the (-g1, sig) pair then has a variable point (68 x 8 witnesses more, 2 in the first one). All zero for
     * the reference's own circuits (params Constant: no witnesses). */
    uint32_t params_mode, off_params_alloc, off_prep_g1;
    /* PublicKeyVar / SignatureVar allocated with AllocationMode::Input (blsw_layout_io; src/constraints.rs:214-249 take any mode): 0 = Witness (the
     * reference's circuits), 1 = Input: the point's x, y, z are public inputs — instance_assignment = [1, pk.x, pk.y, pk.z, sig.x.c0, sig.x.c1,
     * sig.y.c0, sig.y.c1, sig.z.c0, sig.z.c1] in allocation order — and its allocation segment is empty (ark-r1cs-std 0.4.0 allocates Input points
     * through new_variable_omit_prime_order_check: no in-circuit subgroup check, a verifier checks its public inputs itself). Matrix columns:
     * 0 = one, 1 .. n_instance_vars - 1 = the inputs, n_instance_vars + k = witness k.
     * The message allocated with UInt8::new_input_vec (blsw_layout_inputs, msg_mode 1) has no field of its own here: it comes first, as
     * c = ceil(msg_len / 47) public inputs, and the caller recovers c as n_instance_vars - 1 - 3 * pk_mode - 6 * sig_mode. Its segment is then
     * stride_msg = 761 * c witnesses instead of 8 * msg_len.
     * aggregate_verify with Input arguments (blsw_layout_aggregate_inputs, ABI 13) has no field of its own either: pk_mode / sig_mode report the keys' /
     * the signature's mode, the message's mode shows in stride_msg (761 * c instead of 8 * msg_len) and the bitmap's in off_msg == off_bitmap (its segment
     * is empty); off_bitmap == off_keys says the same of the keys. instance_assignment = [1, key_0.x, key_0.y, key_0.z, .., key_{K-1}.z, b_0 .. b_{K-1},
     * m_0 .. m_{c-1}, sig.x.c0 .. sig.z.c1], the selected groups only. */
    uint32_t pk_mode, sig_mode;
} blsw_layout_t;

/* layout(circuit shape) — replaces reading cs.num_witness_variables() after synthesis (constraints.rs:369-373). Host only. */
int blsw_layout(uint32_t msg_len, blsw_layout_t* out);

/* layout of the aggregate_verify circuit with n_keys public keys (keys Witness, bitmap booleans Witness, msg, sig, then
 * mapped_aggregate + verify: src/constraints.rs:153-191, 378-441). n_keys == 0 gives blsw_layout. Host only. */
int blsw_layout_aggregate(uint32_t msg_len, uint32_t n_keys, blsw_layout_t* out);
/* ABI 13: aggregate_verify with each of its four arguments Witness (0, the reference's test) or Input, independently: agg_inputs is a mask of */
#define BLSW_AGG_KEYS_INPUT   1   /* every PublicKeyVar::new_variable(.., Input)            */
#define BLSW_AGG_BITMAP_INPUT 2   /* every Boolean::new_input                               */
#define BLSW_AGG_MSG_INPUT    4   /* UInt8::new_input_vec, as options.msg_mode 1            */
#define BLSW_AGG_SIG_INPUT    8   /* SignatureVar::new_variable(.., Input)                  */
/* Allocation order is the reference test's (constraints.rs:394-441: keys, bitmap, message, parameters Constant, signature), hence the order of the
 * instance variables (blsw_layout_t.pk_mode). An Input key is the pk_mode rule K times: x, y, z instance variables ((0, 1, 0) for the (0, 0) input), no
 * witnesses, no prime-order check; the keys segment is empty. An Input bitmap bit (AllocatedBool::new_variable with Input) is an instance variable that
 * keeps its booleanity constraint (1 - b) * b = 0: no witness, the bitmap segment is empty; select, the additions and addmany of mapped_aggregate
 * allocate what they allocate for witnesses, and count stays a witness (constraints.rs:179). Message and signature as blsw_layout_inputs; the
 * signature's six inputs are the last six, the message chunks sit in front of them. agg_inputs 0 = blsw_layout_aggregate field for field.
 * BLSW_ERR_ARG: agg_inputs > 15, n_keys == 0. Host only. */
int blsw_layout_aggregate_inputs(uint32_t msg_len, uint32_t n_keys, uint32_t agg_inputs, blsw_layout_t* out);
int blsw_aggregate_workspace_bytes(uint64_t n, uint32_t msg_len, uint32_t n_keys, uint64_t* bytes);
/* BlsSignatureVerifyGadget::aggregate_verify for n independent instances of n_keys keys each (same message per instance):
 *   d_pks_xy [n][n_keys][12] u64, d_bitmap [n][n_keys] bytes (0/1: Boolean::new_witness), d_sig_xy [n][24], d_msg [n][msg_len]
 *     (an empty selection and sums that reach the identity are defined inputs; a final sum of O fails the enforced pk != 0 row: tests/test_agg_edges_gpu.py)
 *   d_witness [n][witness_stride] (may be NULL), d_result [n] int32 (the Boolean), d_count [n] uint32 (the UInt32 count)
 * Direct mode, asynchronous on `stream`. */
int blsw_aggregate_verify_batch(const uint64_t* d_pks_xy, const uint8_t* d_bitmap, uint32_t n_keys, const uint64_t* d_sig_xy, const uint8_t* d_msg,
                                uint32_t msg_len, uint64_t n, uint64_t* d_witness, uint64_t witness_stride, int32_t* d_result, uint32_t* d_count,
                                void* d_workspace, uint64_t workspace_bytes, void* stream);

/* N+1-pair product of pairings: ONE signature over n_pairs (pk_j, msg_j) pairs,
 *     e(-g1, sig) * prod_j e(pk_j, H(msg_j)) == 1
 * i.e. BlsSignatureVerifyGadget::verify (src/constraints.rs:90-128) with every per-key statement turned into a loop over the
 * pairs and PairingVar::product_of_pairings called on slices of n_pairs + 1 prepared points (constraints.rs:121-125 passes
 * slices of 2). The reference has no such entry; n_pairs == 1 reproduces the single-key witness vector
 * bit for bit. Circuit allocation order: msg_0..msg_{K-1} witness bytes, params Constant, pk_0..pk_{K-1} Witness, sig Witness.
 *   d_pks_xy [n][n_pairs][12], d_msgs [n][n_pairs][msg_len], d_sig_xy [n][24]
 *   d_witness [n][witness_stride] (may be NULL), d_result [n] int32
 * Direct mode on the device that owns `stream`. The call copies its descriptor to the device and SYNCHRONISES `stream` once
 * before issuing the kernels (asynchronous from there on); side streams are kept per host thread and device. */
int blsw_layout_multi(uint32_t msg_len, uint32_t n_pairs, blsw_layout_t* out);
/* The N+1-pair product with its keys, its messages and its signature Witness (0) or Input, independently: multi_inputs is a mask of */
#define BLSW_MULTI_KEYS_INPUT 1   /* every PublicKeyVar::new_variable(.., Input)            */
#define BLSW_MULTI_MSG_INPUT  4   /* every UInt8::new_input_vec                             */
#define BLSW_MULTI_SIG_INPUT  8   /* SignatureVar::new_variable(.., Input)                  */
/* The values are BLSW_AGG_*_INPUT's; bit 2 (the aggregate circuit's bitmap) means nothing here. Allocation order is the product's own (msgs, params
 * Constant, pks, sig), hence the order of the instance variables, the selected groups only, c = ceil(msg_len / 47):
 *   instance_assignment = [1, m_{0,0} .. m_{0,c-1}, .., m_{K-1,0} .. m_{K-1,c-1}, pk_0.x, pk_0.y, pk_0.z, .., pk_{K-1}.z, sig.x.c0 .. sig.z.c1]
 * Each Input argument is the single-key rule (blsw_layout_inputs), K times: a key is new_variable_omit_prime_order_check — x, y, z instance variables
 * ((0, 1, 0) for the (0, 0) input), no witnesses, the key segments are empty (stride_pk_alloc 0); chunk t of message j is instance variable
 * 1 + j c + t and its to_bits_le is 761 witnesses at off_msg + j * stride_msg + 761 t (stride_msg = 761 c); the signature is six instance variables
 * and an empty allocation segment. n_instance_vars = 1 + (MSG ? K c : 0) + (KEYS ? 3 K : 0) + (SIG ? 6 : 0); n_witness against blsw_layout_multi changes
 * by -1942 K (KEYS), -12413 (SIG), +(761 c - 8 msg_len) K (MSG). pk_mode / sig_mode of the layout report the modes, the message's shows in stride_msg.
 * multi_inputs 0 = blsw_layout_multi field for field; n_pairs 1 = blsw_layout_inputs(msg_len, MSG, KEYS, SIG) field for field.
 * BLSW_ERR_ARG: bit 2 or a value above 15, n_pairs == 0 or > 4096. Host only. */
int blsw_layout_multi_inputs(uint32_t msg_len, uint32_t n_pairs, uint32_t multi_inputs, blsw_layout_t* out);
/* single-key circuit with ParametersVar::new_variable(.., mode) (src/constraints.rs:198-211): params_mode 0 = Constant (blsw_layout),
 * 1 = Witness. AllocationMode::Input would put the generator into instance_assignment, which this engine does not produce:
 * BLSW_ERR_ARG. Host only. */
int blsw_layout_params(uint32_t msg_len, uint32_t params_mode, blsw_layout_t* out);
/* single-key circuit with PublicKeyVar / SignatureVar::new_variable(.., mode) (src/constraints.rs:214-249): pk_mode / sig_mode 0 = Witness, 1 = Input
 * (blsw_layout_t.pk_mode). AllocationMode::Constant for a key or a signature is a different circuit in four segments and is not offered: BLSW_ERR_ARG.
 * Parameters Constant. Host only. */
int blsw_layout_io(uint32_t msg_len, uint32_t pk_mode, uint32_t sig_mode, blsw_layout_t* out);
/* ABI 12: blsw_layout_io with the message's allocation mode as well (src/constraints.rs:341): msg_mode 0 = UInt8::new_witness_vec (= blsw_layout_io),
 * 1 = UInt8::new_input_vec (ark-r1cs-std 0.4.0; packing of ark-ff 0.4's ToConstraintField<Fq> for [u8]). The message is cut into c = ceil(msg_len / 47)
 * chunks of 47 bytes (the last one may be shorter); chunk j, read as a little-endian integer (< 2^376 < p), is public input 1 + j — before the key's and
 * the signature's: instance_assignment = [1, m_0 .. m_{c-1}, pk.x, pk.y, pk.z (pk_mode 1), sig.x.c0 .. sig.z.c1 (sig_mode 1)] — and its
 * AllocatedFp::to_bits_le is the chunk's segment of 761 witnesses (381 booleans LSB first, then enforce_in_field_le's AND witnesses) at
 * off_msg + 761 j. Byte k of the message is bits [8 k, 8 k + 8) of the chunks' low 376 bits concatenated (UInt8::from_bits_le: no variables). msg_len 0:
 * c = 0, the msg_mode 0 circuit. Single-key circuit with Constant parameters, as pk_mode. Host only. */
int blsw_layout_inputs(uint32_t msg_len, uint32_t msg_mode, uint32_t pk_mode, uint32_t sig_mode, blsw_layout_t* out);
int blsw_verify_multi_workspace_bytes(uint64_t n, uint32_t msg_len, uint32_t n_pairs, uint64_t* bytes);
int blsw_verify_multi_batch(const uint64_t* d_pks_xy, const uint8_t* d_msgs, uint32_t msg_len, uint32_t n_pairs, const uint64_t* d_sig_xy, uint64_t n,
                            uint64_t* d_witness, uint64_t witness_stride, int32_t* d_result, void* d_workspace, uint64_t workspace_bytes, void* stream);

/* Execution engine. Batches of n instances are SUBMITTED with their input / output pointers and processed in groups
 * of up to max_steps batches by one set of kernel launches (one batch of 1024 instances is only 16 wavefronts per
 * chain; a group of 16 batches fills a quarter of the 1024 SIMDs of an MI355X per chain kernel and several chains and
 * groups run side by side). max_steps == 1 with n_buffers == 1 is the direct mode: the chains write every witness in
 * place. Otherwise field witnesses are staged (coalesced stores) and each batch's witness tensor is written, in
 * submission order, by two streaming kernels on their own streams: the SHA-256 boolean segment (93 % of the bytes) as
 * soon as the batch's SHA witness bits exist — it does not wait for the curve / pairing chains — and the field segments
 * when the group's chains have finished. n_buffers groups can be in flight at once (each with its own streams and
 * workspace slice). The caller owns the device workspace (blsw_engine_workspace_bytes). Every entry point switches to
 * the engine's device for the duration of the call. One engine per device; not thread-safe.
 * Largest per-lane stack of the default kernels: 4.6 KB (the Fp12 inversion hint of the six-lane pairing kernel). */
typedef struct blsw_engine blsw_engine_t;
typedef struct {
    int32_t device;        /* HIP device ordinal, -1 = the current device */
    uint32_t n_keys;       /* 0 = the single-key circuit (blsw_engine_submit); K > 0 = the aggregate_verify circuit with K keys
                            * (blsw_layout_aggregate; batches go through blsw_engine_submit_aggregate) */
    uint32_t pairing_mode; /* 0 = six lanes per instance (default), 1 = one lane per instance (9.7 KB stack: A/B runs only) */
    uint32_t g2_mode;      /* 0 = one lane per instance (default), 1 = six lanes per instance (needs pairing_mode 0) */
    uint32_t expand_variant; /* store geometry of the SHA expansion kernel, low byte: 0 = 384 threads x 8 pieces, 1 = one 4 KiB-aligned
                              * chunk per 256-thread workgroup, 2 / 3 / 4 = 768 threads x 8 / 4 / 16 pieces in 4 KiB-aligned chunks, 5 = 384 x 16, 6 / 7 = one
                              * 8 / 16 KiB-aligned chunk per 512- / 1024-thread workgroup, 8 / 9 = 384 x 8 / 4 with the bit words in scalar registers
                              * (14 vector registers per lane), 10 / 11 / 12 = 384 x 8 / 16 / 32 with a light instruction stream (scalar bit window, scalar store base: 5 vector
                              * instructions per store instead of ~20), 13 = the blocks of 0 walked by a resident grid of 512 workgroups (a grid that is dispatched at once:
                              * the engine takes it by itself for the expansions it issues beside a latency group's chains); | 0x100 = raised wave priority.
                              * Only 0 is the shipped path. 10 / 11 / 12 (and expand_store 2 / 3) are EXPERIMENTAL, non-default measurement variants: their inline
                              * assembly carries hand-counted hazard wait states for gfx950 (the unit refuses to compile for another target) and only
                              * test_expansion_geometries_bit_exact guards them */
    uint32_t expand_store; /* stores of the SHA expansion kernel: 0 plain (default), 1 nontemporal, 2 sc1, 3 sc0 sc1 (variant 0) */
    uint32_t prio_mode;    /* stream priorities: 0 chains high, 1 placement high (default), 2 equal */
    uint32_t place_lds;    /* optional occupancy limiter of the expansion kernel: bytes of dynamic LDS per workgroup */
    uint32_t consumer_mode; /* 0 (default): free running — a step is written into its output as soon as stream order allows, the
                              caller guarantees that reusing an output is safe; 1: every output (witness tensor or compact buffer)
                              must be released with blsw_engine_output_consumed before its next use, and a step whose output is
                              still held is written later, when it is released (outputs can then be a ring much smaller than
                              the number of steps in flight: the chains run ahead into the staging, the 34 MB vectors exist only
                              between expansion and consumption) */
    uint32_t output_form;  /* witness elements in the output tensors: 0 (default) Montgomery form, 6 little-endian u64 limbs of
                              a * 2^384 mod p — reinterpretable as arkworks' in-memory Fq; 1: canonical integers, 48 bytes
                              little-endian — what CanonicalSerialize writes for an Fq (a prover in another process, a file).
                              The compact wire form is the same for both; blsw_engine_expand_compact follows the expanding
                              engine's option */
    uint32_t chain_variant; /* which compilation of the one-instance-per-lane chain kernels: 0 (default) = out of line in the grouped
                              engine (they leave registers to the streaming kernels that share their SIMDs), inlined in direct mode
                              (max_steps == 1 and n_buffers == 1: shorter under load, the whole register file) and for a small launch
                              group (at most 8 192 lanes) that starts a pipeline — the first two after creation / a flush — whose
                              latency is what a consumer waits for; 1 = out of line; 2 = inlined. Same witnesses either way. */
    uint32_t n_pairs;      /* 0 / 1 = the single-key circuit; K > 1 = the N+1-pair product (blsw_layout_multi): one signature over K (pk, msg)
                              pairs per instance, batches through blsw_engine_submit_multi. Staged engines only (max_steps > 1 or
                              n_buffers > 1), default kernel modes, n * K <= 65535. Compact wire form (blsw_engine_submit_multi_compact,
                              ~180 MB instead of 4.19 GB per instance at K = 128): n * K a multiple of 64 and n a divisor or a multiple of 64 */
    uint32_t cofactor_mode; /* clear_cofactor2 (the longest chain) with the three 255-bit chunks of its scalar on three lanes and a join: half the
                              chain's latency for 38 % more products in it. 0 (default) = for launch groups of at most 8 192 lanes (latency-bound),
                              one chain per lane above; 1 = never; 2 = always. Same witnesses either way. */
    uint32_t params_mode;  /* ParametersVar allocation (src/constraints.rs:198-211): 0 (default) Constant, as in every circuit of the reference;
                              1 Witness (blsw_layout_params): the generator is allocated like a public key, prepare_g1(-g1) and the ell of
                              the (-g1, sig) pair emit witnesses. Single-key circuit with the default kernel modes only (n_keys 0, n_pairs <= 1,
                              pairing_mode 0). */
    uint32_t group_ramp;   /* 0 (default): every launch group is max_steps batches (the last one of a flush: what is pending). 1: the first groups
                              after creation / a flush are 2, 4, 8, ... batches, up to max_steps: the first witness tensors exist after the chain
                              latency of a small group (its cofactor chain on three lanes), which is what a consumer-mode caller waits for
                              before it can consume anything. Same witnesses either way. */
    uint32_t latency_mode; /* the latency kernels for launch groups of at most 8 192 lanes: the hash-to-G2 / prepare / G2-allocation chains of an item on the
                              four lanes of a quad (the independent Fp products of every Fp2 operation on different lanes) and clear_cofactor2 "values
                              first" (the 636 doublings and 304 additions as Jacobian value chains with four inversions in all, every step's witnesses
                              derived by a lane of its own). 0 (default) = for such a group when it finds the engine's chains idle (it starts a pipeline:
                              its latency is what a consumer waits for); 1 = never; 2 = for every such group; 3 / 4 = as 2 with only the values-first
                              cofactor chain / only the quads (A/B runs). Same witnesses either way. */
    uint32_t pk_mode;      /* PublicKeyVar allocation (src/constraints.rs:214-232): 0 (default) Witness, 1 Input (blsw_layout_io): batches go through
                              blsw_engine_submit_io, which also writes instance_assignment. Single-key circuit with Constant parameters only. */
    uint32_t sig_mode;     /* SignatureVar allocation (src/constraints.rs:234-249): 0 (default) Witness, 1 Input; as pk_mode; not with g2_mode 1 */
    uint32_t msg_mode;     /* message allocation (src/constraints.rs:341, ABI 12): 0 (default) UInt8::new_witness_vec, 1 UInt8::new_input_vec (blsw_layout_inputs):
                              blsw_engine_submit_io writes the message chunks into instance_assignment as well. Single-key circuit with Constant parameters
                              and g2_mode 0 only, as pk_mode. */
    uint32_t agg_inputs;   /* aggregate_verify engines (n_keys > 0, ABI 13): mask of BLSW_AGG_*_INPUT (blsw_layout_aggregate_inputs), 0 (default) = every argument
                              Witness. With BLSW_AGG_KEYS_INPUT nothing allocates keys: no allocation kernel runs and the workspace holds no projective keys.
                              blsw_engine_submit_aggregate_io also writes instance_assignment. The aggregate circuit's modes are this mask: pk_mode, sig_mode
                              and msg_mode stay refused together with n_keys. BLSW_ERR_ARG: a value above 15, a non-zero value with n_keys == 0. */
    uint32_t shared_keys;  /* aggregate_verify engines (ABI 15): 0 (default) every step brings its keys [n][K][12] and allocates them per instance; 1 = every step
                              names a key set (blsw_keyset_t below) whose allocation witnesses were computed once: they are copied into the head of every
                              instance's vector and nothing of the keys is staged, kept in the workspace or carried by the compact form. The circuit, the
                              layout (blsw_layout_aggregate_inputs of agg_inputs) and every output element are those of shared_keys 0. Batches go through
                              blsw_engine_submit_aggregate_keyset / _keyset_compact. BLSW_ERR_ARG: a value above 1, n_keys == 0, agg_inputs with
                              BLSW_AGG_KEYS_INPUT (Input keys have no allocation witnesses to share). */
} blsw_engine_options_t;
/* the defaults (pure: measurement scripts set the fields they want to vary). The one environment variable the library reads is the
 * diagnostic BLSW_TRACE_GROUP=1: an engine prints its launch groups' stage times to stderr at blsw_engine_destroy. */
int blsw_engine_options_default(blsw_engine_options_t* out);
int blsw_engine_workspace_bytes(uint64_t n, uint32_t msg_len, uint32_t max_steps, uint32_t n_buffers, uint64_t* bytes);
/* BLSW_ERR_ARG for every argument and option set blsw_engine_create_ex refuses with BLSW_ERR_ARG before it looks at the device */
int blsw_engine_workspace_bytes_ex(uint64_t n, uint32_t msg_len, uint32_t max_steps, uint32_t n_buffers, const blsw_engine_options_t* options, uint64_t* bytes);
/* blsw_engine_create = blsw_engine_create_ex with blsw_engine_options_default. Returns BLSW_ERR_SCRATCH (nothing is
 * allocated) when pairing_mode 1 is combined with so many group buffers that the runtime's per-queue scratch
 * (stack bytes x 64 lanes x wave slots of the device, per queue) would exceed what ROCr can back: that combination
 * used to abort the process with HSA_STATUS_ERROR_OUT_OF_RESOURCES. */
/* BLSW_ERR_ARG also for: n > 65535 (one row of workgroups per instance in the expansion launches; no restriction in practice: a step's
 * output is n witness vectors of 34 MB, so 288 GB of HBM hold steps of at most ~8 000 instances — larger batches are more steps); options->consumer_mode > 1;
 * options->consumer_mode == 1 on a direct-mode engine (max_steps == 1 and n_buffers == 1: it writes witnesses in place while
 * the chains run and cannot hold a step back). */
int blsw_engine_create(blsw_engine_t** out, uint64_t n, uint32_t msg_len, uint32_t max_steps, uint32_t n_buffers, void* d_workspace,
                       uint64_t workspace_bytes);
int blsw_engine_create_ex(blsw_engine_t** out, uint64_t n, uint32_t msg_len, uint32_t max_steps, uint32_t n_buffers, const blsw_engine_options_t* options,
                          void* d_workspace, uint64_t workspace_bytes);
/* An N+1-pair engine whose keys, messages and signature are Witness or Input: blsw_engine_workspace_bytes_ex / blsw_engine_create_ex with the mask
 * multi_inputs (BLSW_MULTI_*_INPUT, blsw_layout_multi_inputs) beside the options. The mask is an argument and not a field of blsw_engine_options_t: the
 * struct, and with it every caller compiled against it, stays as it is. multi_inputs 0 = the _ex functions. A non-zero mask requires options->n_pairs >= 2
 * and none of n_keys, params_mode, pk_mode, sig_mode, msg_mode, agg_inputs, shared_keys (the product's modes are this mask: pk_mode, sig_mode and
 * msg_mode stay refused together with n_pairs > 1), and everything an n_pairs engine requires: staged, default kernel modes, n * n_pairs <= 65535.
 * BLSW_ERR_ARG otherwise, for bit 2 of the mask and for a value above 15; both functions refuse the same sets. Batches go through
 * blsw_engine_submit_multi_io, which also writes instance_assignment. */
int blsw_engine_workspace_bytes_multi_inputs(uint64_t n, uint32_t msg_len, uint32_t max_steps, uint32_t n_buffers, const blsw_engine_options_t* options,
                                             uint32_t multi_inputs, uint64_t* bytes);
int blsw_engine_create_multi_inputs(blsw_engine_t** out, uint64_t n, uint32_t msg_len, uint32_t max_steps, uint32_t n_buffers, const blsw_engine_options_t* options,
                                    uint32_t multi_inputs, void* d_workspace, uint64_t workspace_bytes);
int blsw_engine_destroy(blsw_engine_t* e);
/* blsw_engine_submit for an engine with msg_mode / pk_mode / sig_mode Input (it works for every single-key engine): additionally writes
 * d_instance [n][n_instance_vars][6] u64 = each instance's instance_assignment (element 0 = one; Montgomery limbs, or canonical integers with
 * options.output_form 1), i.e. what ConstraintSystem::instance_assignment holds after synthesis. d_instance may be NULL. */
int blsw_engine_submit_io(blsw_engine_t* e, const uint64_t* d_pk_xy, const uint64_t* d_sig_xy, const uint8_t* d_msg, uint64_t* d_instance, uint64_t* d_witness,
                          uint64_t witness_stride, int32_t* d_result, void* stream);

/* Submits one batch of n independent (pk, msg, sig) instances: the witness vectors of the circuit of
 * src/constraints.rs:335-366 are written to d_witness and the gadget's output Boolean (constraints.rs:127) to d_result.
 *   d_pk_xy   [n][12] u64  affine G1 (x, y) Montgomery; (0,0) = point at infinity      (PublicKeyVar, constraints.rs:214-232)
 *   d_sig_xy  [n][24] u64  affine G2 (x.c0, x.c1, y.c0, y.c1); all zero = infinity     (SignatureVar, constraints.rs:234-249)
 *   d_msg     [n][msg_len] bytes                                                        (UInt8::new_witness_vec, constraints.rs:341)
 *   d_witness [n][witness_stride] field elements (48 B each), witness_stride >= layout.n_witness; may be NULL (results only)
 *   d_result  [n] int32, may be NULL
 * The points are taken as decoded: every curve point is defined input, inside the prime-order subgroup or not (no entry point of the witness
 * path makes a subgroup check, and the circuit's allocations accept such points too); the vector is the circuit's on that point in every engine
 * shape (tests/test_chain_edges_gpu.py). A pair (x, y) that is not on the curve is out of scope: the reference's deserialisation rejects it, so
 * nothing defines its vector.
 * Device work is issued when max_steps batches are pending or at blsw_engine_flush; `stream` (hipStream_t, may be NULL)
 * is the stream on which THIS batch's inputs become valid (recorded per submit). Buffers must stay alive until the
 * step has completed. Steps are numbered 0, 1, 2, ... in submission order (blsw_engine_submitted).
 * Host blocking: the device work is asynchronous, but a submit that starts a new group in a group buffer whose previous group
 * (n_buffers groups back) has not finished writing its outputs WAITS on the host for that group (its staging is about to be
 * overwritten) — with n_buffers groups in flight this is the engine's back-pressure. In consumer mode it returns BLSW_ERR_BUSY
 * instead when that group still has steps held back by unreleased outputs. */
int blsw_engine_submit(blsw_engine_t* e, const uint64_t* d_pk_xy, const uint64_t* d_sig_xy, const uint8_t* d_msg, uint64_t* d_witness,
                       uint64_t witness_stride, int32_t* d_result, void* stream);
/* The same step from COMPRESSED bytes in one call (PublicKey::try_from / Signature::try_from + verify, src/bls.rs:219-242, 316-339 and
 * tests/tests.rs:239-268): d_pk48 [n][48] and d_sig96 [n][96] are decoded on `stream` into d_pk_xy [n][12] / d_sig_xy [n][24]
 * (caller buffers: they are the step's inputs and must stay alive like them; a point that fails to decode, or the identity,
 * becomes all zeros = the default point, as the reference's test substitutes it) with d_status [n][2] as blsw_decode_batch writes
 * it, and the step is submitted. d_result[i] = 1 iff both statuses are BLSW_ST_OK and the gadget's Boolean is true — the
 * verdict of tests/tests.rs:244-263. Witness vectors are written for every instance (for rejected inputs: the defined but
 * unsatisfiable assignment of the default points). BLSW_ERR_BUSY as blsw_engine_submit (nothing is issued then). */
int blsw_engine_submit_bytes(blsw_engine_t* e, const uint8_t* d_pk48, const uint8_t* d_sig96, const uint8_t* d_msg, uint64_t* d_pk_xy, uint64_t* d_sig_xy,
                             int32_t* d_status, uint64_t* d_witness, uint64_t witness_stride, int32_t* d_result, void* stream);
/* aggregate_verify (src/constraints.rs:153-191) through the engine, for an engine created with options.n_keys = K: one batch of n
 * instances of K keys each, same grouping / staging / streaming placement as blsw_engine_submit.
 *   d_pks_xy [n][K][12] u64, d_bitmap [n][K] bytes (0/1), d_sig_xy [n][24], d_msg [n][msg_len]
 *   d_witness [n][witness_stride] (stride >= blsw_layout_aggregate().n_witness; may be NULL), d_result [n] int32, d_count [n] uint32 (may be NULL) */
int blsw_engine_submit_aggregate(blsw_engine_t* e, const uint64_t* d_pks_xy, const uint8_t* d_bitmap, const uint64_t* d_sig_xy, const uint8_t* d_msg,
                                 uint64_t* d_witness, uint64_t witness_stride, int32_t* d_result, uint32_t* d_count, void* stream);
/* blsw_engine_submit_aggregate for an engine with options.agg_inputs (it works for every aggregate engine, mask 0 included: then it writes [1]):
 * additionally writes d_instance [n][n_instance_vars][6] u64 = each instance's instance_assignment (element 0 = one; Montgomery limbs, or canonical
 * integers with options.output_form 1); d_instance may be NULL. blsw_engine_submit_aggregate and blsw_engine_submit_aggregate_compact work on an engine
 * with a non-zero mask and write no instance vector (the compact form carries witnesses only). BLSW_ERR_ARG on a single-key engine.
 * The direct call blsw_aggregate_verify_batch has no options and stays all-Witness; a direct-mode engine is the direct path of these shapes. */
int blsw_engine_submit_aggregate_io(blsw_engine_t* e, const uint64_t* d_pks_xy, const uint8_t* d_bitmap, const uint64_t* d_sig_xy, const uint8_t* d_msg,
                                    uint64_t* d_instance, uint64_t* d_witness, uint64_t witness_stride, int32_t* d_result, uint32_t* d_count, void* stream);
/* The N+1-pair product (blsw_verify_multi_batch's circuit) through the engine, for an engine created with options.n_pairs = K: one
 * batch of n instances, same grouping / staging / streaming placement / consumer mode as blsw_engine_submit — more instances are in
 * flight than output tensors exist (a vector is 4.19 GB at K = 128), which the direct call cannot do.
 *   d_pks_xy [n][K][12] u64, d_msgs [n][K][msg_len] bytes, d_sig_xy [n][24]
 *   d_witness [n][witness_stride] (stride >= blsw_layout_multi().n_witness; may be NULL), d_result [n] int32 */
int blsw_engine_submit_multi(blsw_engine_t* e, const uint64_t* d_pks_xy, const uint8_t* d_msgs, const uint64_t* d_sig_xy, uint64_t* d_witness,
                             uint64_t witness_stride, int32_t* d_result, void* stream);
/* blsw_engine_submit_multi for an engine created with blsw_engine_create_multi_inputs (it works for every N+1-pair engine, mask 0 included: then the witness is
 * blsw_engine_submit_multi's bit for bit and it writes [1]): additionally writes d_instance [n][n_instance_vars][6] u64 = each instance's
 * instance_assignment (element 0 = one; Montgomery limbs, or canonical integers with options.output_form 1); d_instance may be NULL.
 * blsw_engine_submit_multi, blsw_engine_submit_multi_compact and blsw_engine_expand_compact work on an engine with a non-zero mask and write no
 * instance vector (the compact form carries witnesses only). BLSW_ERR_ARG on an engine with n_pairs < 2. */
int blsw_engine_submit_multi_io(blsw_engine_t* e, const uint64_t* d_pks_xy, const uint8_t* d_msgs, const uint64_t* d_sig_xy, uint64_t* d_instance, uint64_t* d_witness,
                                uint64_t witness_stride, int32_t* d_result, void* stream);
/* Issues everything pending and makes `stream` wait for all batches submitted so far (asynchronous for the host). In consumer
 * mode: for all steps written so far (blsw_engine_materialised); the rest follow as their outputs are released. */
int blsw_engine_flush(blsw_engine_t* e, void* stream);
/* Streaming consumers (a prover draining witness tensors through a small ring of output buffers):
 *   blsw_engine_submitted / _launched / _materialised: number of steps submitted / whose chains are issued to the device /
 *   whose output writes are issued (equal to launched unless options.consumer_mode holds steps back);
 *   blsw_engine_wait_step: makes `stream` wait until step `seq` has written its output and results (seq < launched;
 *   BLSW_ERR_BUSY while seq >= materialised);
 *   blsw_engine_output_consumed: records on `stream` that the consumer is done with the output at d_output (witness tensor or
 *   compact buffer); the next step submitted with the same pointer does not overwrite it before that point.
 * consumer_mode 0: that release must have been recorded before the group containing the next user of the output is launched
 * (max_steps <= ring). consumer_mode 1: no such rule — steps are written into their outputs in submission order, each as soon
 * as its output has been released; blsw_engine_submit returns BLSW_ERR_BUSY instead of blocking when the group buffer it needs
 * still has unwritten steps (drain: wait_step + output_consumed of the materialised steps, then submit again).
 * At most 64 distinct output pointers may have a pending release, a held step or an accepted (not yet written) step at one time:
 * a consumer-mode submit reserves its output's slot BEFORE the step is taken and returns BLSW_ERR_BUSY with nothing queued or
 * launched when the table is full, and so does blsw_engine_output_consumed for an output the table has no slot for (releases whose
 * event has completed are recycled: release / drain and call again). */
int blsw_engine_submitted(blsw_engine_t* e, uint64_t* seq);
int blsw_engine_launched(blsw_engine_t* e, uint64_t* seq);
int blsw_engine_materialised(blsw_engine_t* e, uint64_t* seq);
int blsw_engine_wait_step(blsw_engine_t* e, uint64_t seq, void* stream);
int blsw_engine_output_consumed(blsw_engine_t* e, const void* d_output, void* stream);
/* Compact wire form of a step, for the multi-GPU all-gather of witness shards: the full vectors are 34 MB per
 * instance and 94 % of their elements are SHA-256 booleans, so every rank receiving the other ranks' shards over xGMI caps an
 * 8-GPU job far below the generation rate. In compact form a batch is its bit-packed SHA witnesses plus its field witnesses as
 * 48-byte elements (2.6 MB per instance: blsw_engine_compact_bytes per batch); that is what travels, and the receiver turns it
 * into the n witness vectors — bit-exact what blsw_engine_submit writes — with blsw_engine_expand_compact. Engines with
 * n % 64 == 0 and (max_steps > 1 or n_buffers > 1).
 *   blsw_engine_submit_compact: as blsw_engine_submit, the step's output is d_compact (compact_bytes bytes) instead of d_witness;
 *     blsw_engine_wait_step / _output_consumed (with the d_compact pointer) work as for witness tensors;
 *   blsw_engine_expand_compact: enqueues on `stream` the expansion of one compact batch (produced by ANY engine of the same
 *     n, msg_len and options, e.g. another rank's) into d_witness [n][witness_stride]. */
int blsw_engine_compact_bytes(blsw_engine_t* e, uint64_t* bytes);
int blsw_engine_submit_compact(blsw_engine_t* e, const uint64_t* d_pk_xy, const uint64_t* d_sig_xy, const uint8_t* d_msg, void* d_compact, int32_t* d_result,
                               void* stream);
/* the same for an aggregate_verify engine (options.n_keys = K): arguments of blsw_engine_submit_aggregate, output d_compact */
int blsw_engine_submit_aggregate_compact(blsw_engine_t* e, const uint64_t* d_pks_xy, const uint8_t* d_bitmap, const uint64_t* d_sig_xy, const uint8_t* d_msg,
                                         void* d_compact, int32_t* d_result, uint32_t* d_count, void* stream);
/* the same for an N+1-pair engine (options.n_pairs = K): arguments of blsw_engine_submit_multi, output d_compact (blsw_engine_compact_bytes bytes);
 * blsw_engine_expand_compact turns it into the n vectors of 4.19 GB (K = 128) on the receiver */
int blsw_engine_submit_multi_compact(blsw_engine_t* e, const uint64_t* d_pks_xy, const uint8_t* d_msgs, const uint64_t* d_sig_xy, void* d_compact, int32_t* d_result,
                                     void* stream);
int blsw_engine_expand_compact(blsw_engine_t* e, const void* d_compact, uint64_t* d_witness, uint64_t witness_stride, void* stream);
/* ABI 14: where a witness element lives in a compact buffer — what a consumer needs to read a step without expanding it (blsw_r1cs_check_compact).
 * A compact step of n instances (n a multiple of 64; instance i is lane i & 63 of tile i / 64) is three regions back to back:
 *   bit words   [n/64][sha_words/16][64][16] u32 at offset 0: witness off_expand + b (b < sha_bits) is bit b & 31 of word b / 32 of the lane's stream
 *   tile rows   [n/64][split_row][64] elements at off_staging: staged row r < split_row of a lane
 *   pair rows   [n][pair_rows] elements at off_pair: staged row split_row + r of a lane (the pairing segments, instance-major)
 * Staged rows are the witness vector with the SHA segment cut out (staging_rows = n_witness - sha_bits); with options.g2_mode 1 the moved_len
 * witnesses from moved_lo on are staged last, from row moved_at on (moved_len 0 otherwise). Elements are always Montgomery form.
 * The N+1-pair product's compact form (pair tiles and instance tiles) is described by blsw_compact_layout_multi_t below, not by this struct. */
typedef struct {
    uint64_t n, off_staging, off_pair, total; /* instances of the step; byte offsets of the two row regions; bytes of the step */
    uint32_t n_witness, off_expand, sha_bits, sha_words, split_row, staging_rows, pair_rows, moved_lo, moved_len, moved_at;
} blsw_compact_layout_t;
#define BLSW_COMPACT_BIT 0  /* regions blsw_compact_locate reports */
#define BLSW_COMPACT_TILE 1
#define BLSW_COMPACT_PAIR 2
/* The layout of the compact steps of an engine created with (n, msg_len, options) — any staged engine: max_steps and n_buffers do not enter.
 * total == blsw_engine_compact_bytes of such an engine. BLSW_ERR_ARG: a NULL pointer, n % 64 != 0, options.n_pairs > 1, and every option set
 * blsw_engine_create_ex refuses for a staged engine. Host only. */
int blsw_compact_layout(uint64_t n, uint32_t msg_len, const blsw_engine_options_t* options, blsw_compact_layout_t* out);
/* witness k (< n_witness) of instance `lane` (< n) of a compact step: *region = BLSW_COMPACT_*; *byte_offset = offset in the buffer of the u32 word
 * that holds the bit (then *bit = its position in the word, LSB = 0) or of the element's 48 bytes (*bit = 0). The one statement of the rule:
 * the device checker evaluates the same function. BLSW_ERR_ARG: a NULL pointer, k or lane out of range, an inconsistent layout. Host only. */
int blsw_compact_locate(const blsw_compact_layout_t* layout, uint32_t k, uint64_t lane, uint32_t* region, uint64_t* byte_offset, uint32_t* bit);
/* ABI 15: a key set shared by many aggregate_verify instances (a committee that signs many messages: only bitmap, message and signature change).
 * The allocation witnesses of its K keys — SEG 1 942 elements per key, G1Var::new_variable(Witness) with its in-circuit prime-order check, what
 * blsw_engine_submit_aggregate computes per (instance, key) — are computed ONCE into a device table; an engine with options.shared_keys copies the
 * table into elements [0, K * 1942) of every instance's vector (off_keys == 0) and reads the K allocated projective keys for mapped_aggregate.
 * Conventions of blsw_r1cs_create: the caller owns d_buffer (256-byte aligned, blsw_keyset_bytes bytes), which must outlive the handle AND every step
 * submitted with it; device -1 = the current device; create is asynchronous on `stream` (it copies nothing from the host) and every rule is checked on
 * the host before any HIP call. A step that uses the set must be submitted on `stream`, or on a stream ordered behind the create.
 *   d_pks_xy [K][12] u64 affine Montgomery, (0, 0) = the point at infinity;  output_form as blsw_engine_options_t.output_form: the table's element form
 *   blsw_keyset_table: the table [K * 1942][6] u64 (key k at element k * 1942, allocation order) in that form
 * BLSW_ERR_ARG: a NULL handle / key / buffer / output pointer, n_keys == 0 or above 65535, output_form > 1, a misaligned d_buffer, buffer_bytes below
 * blsw_keyset_bytes. */
typedef struct blsw_keyset blsw_keyset_t;
int blsw_keyset_bytes(uint32_t n_keys, uint64_t* bytes);
int blsw_keyset_create(blsw_keyset_t** out, const uint64_t* d_pks_xy, uint32_t n_keys, uint32_t output_form, int32_t device, void* d_buffer, uint64_t buffer_bytes,
                       void* stream);
int blsw_keyset_table(const blsw_keyset_t* ks, const uint64_t** d_table, uint64_t* n_elements);
int blsw_keyset_destroy(blsw_keyset_t* ks);
/* blsw_engine_submit_aggregate_io / _aggregate_compact / blsw_engine_expand_compact for an engine with options.shared_keys: the step's keys are `ks`
 * (per STEP: the steps of one launch group may name different sets), everything else as there. d_instance may be NULL. The compact form carries no key
 * rows (blsw_engine_compact_bytes is smaller by n * K * 1942 * 48 bytes): the receiver supplies the set when it expands. BLSW_ERR_ARG: an engine
 * without shared_keys, a NULL set, a set whose n_keys, output_form or device differ from the engine's. The entry points that take d_pks_xy
 * (blsw_engine_submit_aggregate, _io, _compact) and blsw_engine_expand_compact refuse an engine with shared_keys; blsw_compact_layout refuses the
 * option: its struct describes the buffer, and a shared-keys step's buffer is not the whole witness vector. blsw_compact_layout_keyset (ABI 16,
 * below) gives the buffer's layout and the length of the head, and blsw_r1cs_check_compact_keyset checks such a step from the two. */
int blsw_engine_submit_aggregate_keyset(blsw_engine_t* e, const blsw_keyset_t* ks, const uint8_t* d_bitmap, const uint64_t* d_sig_xy, const uint8_t* d_msg,
                                        uint64_t* d_instance, uint64_t* d_witness, uint64_t witness_stride, int32_t* d_result, uint32_t* d_count, void* stream);
int blsw_engine_submit_aggregate_keyset_compact(blsw_engine_t* e, const blsw_keyset_t* ks, const uint8_t* d_bitmap, const uint64_t* d_sig_xy, const uint8_t* d_msg,
                                                void* d_compact, int32_t* d_result, uint32_t* d_count, void* stream);
int blsw_engine_expand_compact_keyset(blsw_engine_t* e, const blsw_keyset_t* ks, const void* d_compact, uint64_t* d_witness, uint64_t witness_stride, void* stream);
/* Same-box rate of the head broadcast alone (the kernel a shared_keys step runs beside its expansion): the set's table copied into the heads of
 * d_witness [n][witness_stride] (overwritten; witness_stride >= K * 1942), `reps` passes after one warm-up pass on the NULL stream of the set's device;
 * bytes WRITTEN per second, to be read beside blsw_fill_rate. order: 0 = consecutive workgroups take the same table chunk for different instances (what
 * the engine launches), 1 = consecutive workgroups walk the chunks of one instance. Synchronous. */
int blsw_keyset_broadcast_rate(const blsw_keyset_t* ks, uint64_t* d_witness, uint64_t witness_stride, uint64_t n, uint32_t order, uint32_t reps, double* bytes_per_s);
/* average duration (ms) of the bit->Fp expansion kernel launches issued since the previous call (HIP events on the stream they
 * ran on, at most 1024 launches); blocks until they have finished and resets the statistics */
int blsw_engine_expand_stats(blsw_engine_t* e, uint32_t* count, float* avg_ms);

/* Position-dependent, order-independent 128-bit digest of each instance's witness vector (the consumer-side check of the
 * sharded runs). With x_j the little-endian u32 words of the instance's n_witness * 12 words, 16-byte
 * piece q = (x_4q, x_4q+1, x_4q+2, x_4q+3), key_q = (q + 1) * 0x9E3779B1 mod 2^32 and A = 0x85EBCA6B (all sums of 32-bit words mod 2^32,
 * products 32 x 32 -> 64 bits):
 *     d[0] = sum_q (x_4q + key_q) * (x_4q+1 + key_q + A) + (x_4q+2 + key_q + 2 A) * (x_4q+3 + key_q + 3 A)   mod 2^64
 *            (the NH family of UMAC with a position-derived key: one multiply per 8 bytes)
 *     d[1] = lo | hi << 32,  lo = sum_q (x_4q ^ key_q) + (x_4q+2 ^ ~key_q),  hi = sum_q (x_4q+1 ^ key_q) + (x_4q+3 ^ ~key_q)   mod 2^32
 *   (ABI 9; ABI <= 8 summed a splitmix64 finalizer per u64 word: four 64-bit multiplies per 16 bytes made the kernel VALU-bound.)
 *   d_witness [n][witness_stride] elements, d_digest [n][2] u64, any n (launched in slices of 65 535 instances). Reads the tensor once at HBM speed. */
int blsw_witness_digest(const uint64_t* d_witness, uint64_t witness_stride, uint64_t n, uint32_t n_witness, uint64_t* d_digest, void* stream);

/* Constraint matrices (host only, no GPU): the R1CS whose witness vectors the entry points above fill, in arkworks'
 * ConstraintMatrices shape — what `cs.to_matrices()` returns after synthesising the circuit (the reference only prints the
 * system's size, src/constraints.rs:369-373). Constraint i is <A_i, z> * <B_i, z> = <C_i, z> with z = [1] ++ witness; column 0
 * is the constant one, column k is witness k - 1 (n_instance_vars = 1: the gadget allocates no public input). Rows are stored
 * CSR: row i of matrix m occupies entries [row_ptr[m][i], row_ptr[m][i + 1]) of col[m] / val[m] (val: 6 u64 Montgomery limbs
 * per entry), columns ascending, no zero coefficients. Circuit shape: (msg_len, n_keys, n_pairs) as blsw_layout (0, 1),
 * blsw_layout_aggregate (n_keys, 1) and blsw_layout_multi (0, n_pairs). Synthesised symbolically from the product's own
 * statement of the arkworks allocation rules (csrc/r1cs.cpp), independent of witness values: emit once per shape.
 * Usage: blsw_matrices_info -> allocate (n_constraints + 1) row pointers and nnz[m] entries per matrix -> blsw_matrices_fill. */
typedef struct {
    uint64_t n_constraints, n_instance_vars, n_witness;
    uint64_t nnz[3]; /* non-zeros of A, B, C */
} blsw_matrices_info_t;
typedef struct {
    uint64_t* row_ptr[3]; /* [n_constraints + 1] each */
    uint32_t* col[3];     /* [nnz[m]] */
    uint64_t* val[3];     /* [nnz[m]][6] */
} blsw_matrices_t;
int blsw_matrices_info(uint32_t msg_len, uint32_t n_keys, uint32_t n_pairs, blsw_matrices_info_t* out);
int blsw_matrices_fill(uint32_t msg_len, uint32_t n_keys, uint32_t n_pairs, const blsw_matrices_info_t* info, blsw_matrices_t* out);
/* the same for the single-key circuit of blsw_layout_params (params_mode 0 = the two calls above with n_keys 0, n_pairs 1) */
int blsw_matrices_info_params(uint32_t msg_len, uint32_t params_mode, blsw_matrices_info_t* out);
int blsw_matrices_fill_params(uint32_t msg_len, uint32_t params_mode, const blsw_matrices_info_t* info, blsw_matrices_t* out);
/* the same for the single-key circuit of blsw_layout_io: info->n_instance_vars = 1 + the number of public-input field elements; column numbering as in
 * blsw_layout_t.pk_mode (ark-relations' ConstraintMatrices: instance variables first, then the witnesses) */
int blsw_matrices_info_io(uint32_t msg_len, uint32_t pk_mode, uint32_t sig_mode, blsw_matrices_info_t* out);
int blsw_matrices_fill_io(uint32_t msg_len, uint32_t pk_mode, uint32_t sig_mode, const blsw_matrices_info_t* info, blsw_matrices_t* out);
/* the same for the circuit of blsw_layout_inputs (ABI 12); msg_mode 0 = the two calls above */
int blsw_matrices_info_inputs(uint32_t msg_len, uint32_t msg_mode, uint32_t pk_mode, uint32_t sig_mode, blsw_matrices_info_t* out);
int blsw_matrices_fill_inputs(uint32_t msg_len, uint32_t msg_mode, uint32_t pk_mode, uint32_t sig_mode, const blsw_matrices_info_t* info, blsw_matrices_t* out);
/* the same for the circuit of blsw_layout_aggregate_inputs (ABI 13): columns as everywhere (one, the inputs in allocation order, the witnesses);
 * agg_inputs 0 = blsw_matrices_info / _fill (msg_len, n_keys, 1) */
int blsw_matrices_info_aggregate_inputs(uint32_t msg_len, uint32_t n_keys, uint32_t agg_inputs, blsw_matrices_info_t* out);
int blsw_matrices_fill_aggregate_inputs(uint32_t msg_len, uint32_t n_keys, uint32_t agg_inputs, const blsw_matrices_info_t* info, blsw_matrices_t* out);
/* The N+1-pair product with the allocation modes of blsw_layout_multi_inputs; columns: 0 = one, then the inputs in that layout's order, then the
 * witnesses. multi_inputs 0 = blsw_matrices_info / _fill (msg_len, 0, n_pairs) */
int blsw_matrices_info_multi_inputs(uint32_t msg_len, uint32_t n_pairs, uint32_t multi_inputs, blsw_matrices_info_t* out);
int blsw_matrices_fill_multi_inputs(uint32_t msg_len, uint32_t n_pairs, uint32_t multi_inputs, const blsw_matrices_info_t* info, blsw_matrices_t* out);

/* Device R1CS evaluator (ABI 11): checks and evaluates the matrices above against witness vectors on the GPU — arkworks'
 * cs.is_satisfied() / cs.which_is_unsatisfied() and the A z, B z, C z a prover computes first, for n instances at a time.
 * A handle is built once per circuit shape from the host CSR blsw_matrices_fill* wrote: create validates and encodes it (every entry a u32
 * column and a u32 code: +-v for |coefficient| < 2^30, else an index into a table of the distinct Montgomery coefficients; rows cut into
 * blocks of about equal work) into the caller's device buffer (256-byte aligned) of blsw_r1cs_device_bytes bytes, which must outlive the handle.
 * Element form and strides:
 *   z = [instance | witness], columns numbered as in blsw_matrices_info_io (0 = the constant one, then the public inputs, then witness k at
 *   n_instance_vars + k). d_witness [n][witness_stride] and d_instance [n][instance_stride] elements of 6 u64 (strides in field elements,
 *   witness_stride >= n_witness, instance_stride >= n_instance_vars) — the layout blsw_engine_submit / blsw_engine_submit_io write.
 *   form: 0 = Montgomery (the engine's default), 1 = canonical integers (options.output_form 1); every input element in that form.
 *   n_instance_vars == 1: d_instance may be NULL, the constant one is then R mod p (form 0) or 1 (form 1). n_instance_vars > 1: required.
 *   The check assumes reduced elements (< p); blsw_r1cs_check reports the first unreduced one on request.
 * Every argument rule is checked on the host before any HIP call: BLSW_ERR_ARG for a row_ptr that does not start at 0, decreases or
 * does not end at nnz, columns not strictly ascending within a row or not below n_instance_vars + n_witness, a zero coefficient or one
 * >= p, form > 1, n == 0, a stride below the element count, a missing instance vector, a row range outside the matrix.
 * Calls are asynchronous on `stream` (hipStream_t) and run on the handle's device; results leave through vector stores and global atomics. */
typedef struct blsw_r1cs blsw_r1cs_t;
int blsw_r1cs_device_bytes(const blsw_matrices_info_t* info, const blsw_matrices_t* m, uint64_t* bytes);
/* device: HIP ordinal, -1 = the current device. The encoding is copied on `stream`; create synchronises it before it returns. */
int blsw_r1cs_create(blsw_r1cs_t** out, const blsw_matrices_info_t* info, const blsw_matrices_t* m, int32_t device, void* d_buffer, uint64_t buffer_bytes,
                     void* stream);
int blsw_r1cs_destroy(blsw_r1cs_t* r);
/* d_first_unsatisfied [n] int64: index of the first constraint j with <A_j, z> * <B_j, z> != <C_j, z>, or -1 when z satisfies the system.
 * d_first_unreduced [n] int64 (may be NULL): the first index k of z with z_k >= p, or -1. */
int blsw_r1cs_check(blsw_r1cs_t* r, const uint64_t* d_instance, uint64_t instance_stride, const uint64_t* d_witness, uint64_t witness_stride, uint64_t n,
                    uint32_t form, int64_t* d_first_unsatisfied, int64_t* d_first_unreduced, void* stream);
/* rows [row_begin, row_begin + row_count): d_az / d_bz / d_cz [n][row_count][6] u64 = <A_j, z>, <B_j, z>, <C_j, z> reduced, in the input's form */
int blsw_r1cs_evaluate(blsw_r1cs_t* r, const uint64_t* d_instance, uint64_t instance_stride, const uint64_t* d_witness, uint64_t witness_stride, uint64_t n,
                       uint32_t form, uint64_t row_begin, uint64_t row_count, uint64_t* d_az, uint64_t* d_bz, uint64_t* d_cz, void* stream);
/* ABI 14: the same two calls with z read straight from a step's compact buffer (blsw_compact_layout_t above; d_compact 16-byte aligned, layout->total
 * bytes) instead of from expanded witness vectors: n = layout->n instances, results and conventions as blsw_r1cs_check / _evaluate. A receiver validates
 * a step without blsw_engine_expand_compact and without the 34 MB-per-instance tensor. The compact form carries witnesses only: d_instance
 * [n][instance_stride] as above (required when n_instance_vars > 1). Elements are Montgomery form (form 0). d_first_unreduced reads the staged rows
 * only (a bit cannot be unreduced) and reports n_instance_vars + k for witness k. BLSW_ERR_ARG before any launch, nothing written: a NULL handle,
 * layout, buffer or output, layout->n_witness != the handle's, n % 64 != 0 or an inconsistent layout, a missing instance vector or
 * instance_stride < n_instance_vars, a row range outside the matrix. */
int blsw_r1cs_check_compact(blsw_r1cs_t* r, const blsw_compact_layout_t* layout, const void* d_compact, const uint64_t* d_instance, uint64_t instance_stride,
                            int64_t* d_first_unsatisfied, int64_t* d_first_unreduced, void* stream);
int blsw_r1cs_evaluate_compact(blsw_r1cs_t* r, const blsw_compact_layout_t* layout, const void* d_compact, const uint64_t* d_instance, uint64_t instance_stride,
                               uint64_t row_begin, uint64_t row_count, uint64_t* d_az, uint64_t* d_bz, uint64_t* d_cz, void* stream);
/* ABI 16: a shared-keys step (options.shared_keys, ABI 15) checked from its compact buffer plus the receiver's key set, and the committee checked once
 * per set instead of once per instance.
 * The buffer of such a step is the compact form of the rows the engine computes — the circuit without its keys segment, field for field the layout
 * of agg_inputs | BLSW_AGG_KEYS_INPUT — so blsw_compact_layout_t describes it unchanged; the head is the set's table and travels nowhere.
 *   blsw_compact_layout_keyset: options->shared_keys must be 1, otherwise the rules of blsw_compact_layout. *rows = the layout of the buffer
 *     (rows->total == blsw_engine_compact_bytes of such an engine; rows->n_witness = the caller-visible witness count - *head_len);
 *     *head_len = n_keys * 1942. Witness k of the caller's vector is table[k] for k < *head_len, else blsw_compact_locate(rows, k - *head_len, lane).
 *     Host only.
 *   blsw_r1cs_head_rows: the number of leading constraints whose every column is 0 or in [n_instance_vars, n_instance_vars + head_len) — the rows
 *     that are a function of the head alone (1 939 per key of the aggregate circuit: 1 939 * K for head_len = K * 1942). head_len 0 gives 0.
 *     BLSW_ERR_ARG: a NULL pointer, a CSR blsw_r1cs_create refuses, head_len > n_witness. Host only. blsw_r1cs_handle_head_rows answers the same
 *     for the matrices a handle was created from (create keeps the smallest covering head_len of every leading row on the host, not the CSR).
 *   blsw_r1cs_check_keyset: the committee, once — rows [0, P) on z = [1 | table], P = the head rows of the set's n_keys * 1942 elements. The table
 *     may be in either element form (blsw_keyset_create's output_form). d_first_unsatisfied [1] as blsw_r1cs_check; d_first_unreduced [1] (may be
 *     NULL): the first table element >= p, reported as n_instance_vars + k. BLSW_ERR_ARG: a NULL handle, set or output, a set on another device
 *     than the handle, a table longer than the handle's witness count.
 *   blsw_r1cs_check_compact_keyset / _evaluate_compact_keyset: blsw_r1cs_check_compact / _evaluate_compact with z = [instance | table | buffer].
 *     head_rows_mode BLSW_R1CS_HEAD_CHECK: every row for every instance; the verdict is that of blsw_r1cs_check on the step's expansion
 *     (blsw_engine_expand_compact_keyset). BLSW_R1CS_HEAD_SKIP: rows [P, n_constraints) only, reported as they are numbered in the matrix — the
 *     caller vouches for the set with blsw_r1cs_check_keyset (once per set, not per step). d_first_unreduced covers the instance vector and the
 *     staged rows of the buffer, reported at n_instance_vars + head_len + k for the buffer's witness k; it NEVER covers the head, in either
 *     mode: that is blsw_r1cs_check_keyset's. The evaluation takes any row window, head rows included.
 *     BLSW_ERR_ARG before any HIP call, nothing written: every rule of the ABI 14 calls, a NULL set, a set on another device than the handle,
 *     rows_layout->n_witness + n_keys * 1942 != the handle's witness count, head_rows_mode > 1, a set whose table is not Montgomery form
 *     (output_form 1: the buffer's elements never are canonical). */
#define BLSW_R1CS_HEAD_CHECK 0
#define BLSW_R1CS_HEAD_SKIP 1
int blsw_compact_layout_keyset(uint64_t n, uint32_t msg_len, const blsw_engine_options_t* options, blsw_compact_layout_t* rows, uint32_t* head_len);
int blsw_r1cs_head_rows(const blsw_matrices_info_t* info, const blsw_matrices_t* m, uint64_t head_len, uint64_t* rows);
int blsw_r1cs_handle_head_rows(const blsw_r1cs_t* r, uint64_t head_len, uint64_t* rows);
int blsw_r1cs_check_keyset(blsw_r1cs_t* r, const blsw_keyset_t* ks, int64_t* d_first_unsatisfied, int64_t* d_first_unreduced, void* stream);
int blsw_r1cs_check_compact_keyset(blsw_r1cs_t* r, const blsw_compact_layout_t* rows_layout, const void* d_compact, const blsw_keyset_t* ks, uint32_t head_rows_mode,
                                   const uint64_t* d_instance, uint64_t instance_stride, int64_t* d_first_unsatisfied, int64_t* d_first_unreduced, void* stream);
int blsw_r1cs_evaluate_compact_keyset(blsw_r1cs_t* r, const blsw_compact_layout_t* rows_layout, const void* d_compact, const blsw_keyset_t* ks, const uint64_t* d_instance,
                                      uint64_t instance_stride, uint64_t row_begin, uint64_t row_count, uint64_t* d_az, uint64_t* d_bz, uint64_t* d_cz, void* stream);
/* The N+1-pair product's compact form, described, and a step checked straight from it (new symbols; the ABI number is unchanged).
 * A compact step of n instances of K = n_pairs pairs (n K a multiple of 64, n a divisor or a multiple of 64) is four regions back to back; pair j of
 * instance i is PAIR LANE p = i K + j, lane p & 63 of pair tile p / 64:
 *   bit words       [n K / 64][sha_words/16][64][16] u32 at offset 0: witness off_expand + j stride_hash + b (b < sha_bits) is bit b & 31 of word b / 32
 *                   of pair lane p's stream
 *   pair tiles      [n K / 64][rows_p][64] elements at off_staging: staged row e < rows_p of a pair lane. Row e of run r (pair_run_row[r] <= e <
 *                   pair_run_row[r] + pair_run_len[r]) is witness pair_run_off[r] + j pair_run_stride[r] + (e - pair_run_row[r]). The six runs, in row
 *                   order: message, key allocation, pk != 0, hash_to_g2 behind its SHA bits, prepare(H), prepare(pk); a run may be empty (len 0)
 *   instance tiles  [ceil(n / 64)][rows_i][inst_tile_w] elements at off_inst, inst_tile_w = 64 or n (a step that is a part of one tile): staged row e of
 *                   instance lane i, at lane i % inst_tile_w of tile i / inst_tile_w. The two runs: signature allocation, prepare(sig) (inst_run_*)
 *   instance rows   [n][pair_rows] elements at off_pair: witness off_miller + r of instance i (Miller loop, final exponentiation, is_one)
 * Elements are always Montgomery form. */
typedef struct {
    uint64_t n, off_staging, off_inst, off_pair, total; /* instances of the step; byte offsets of the three row regions; bytes of the step */
    uint32_t n_pairs, n_witness, sha_bits, sha_words, off_expand, stride_hash, rows_p, rows_i, pair_rows, inst_tile_w, off_miller, reserved;
    uint32_t pair_run_row[6], pair_run_off[6], pair_run_stride[6], pair_run_len[6];
    uint32_t inst_run_row[2], inst_run_off[2], inst_run_len[2];
} blsw_compact_layout_multi_t;
#define BLSW_COMPACT_INST 3 /* the fourth region blsw_compact_locate_multi reports: an instance tile (BLSW_COMPACT_TILE: a pair tile; _PAIR: the instance rows) */
/* The layout of the compact steps of an engine created with blsw_engine_create_multi_inputs(n, msg_len, .., options, multi_inputs, ..) — any staged
 * engine. total == blsw_engine_compact_bytes of such an engine. BLSW_ERR_ARG: a NULL pointer, options.n_pairs < 2, a shape that cannot leave in compact
 * form (n K % 64 != 0, or n neither a divisor nor a multiple of 64), and every option or mask set blsw_engine_create_multi_inputs refuses for a staged
 * engine. blsw_compact_layout keeps refusing n_pairs > 1. Host only. */
int blsw_compact_layout_multi(uint64_t n, uint32_t msg_len, const blsw_engine_options_t* options, uint32_t multi_inputs, blsw_compact_layout_multi_t* out);
/* witness k (< n_witness) of instance `instance` (< n): *region = BLSW_COMPACT_BIT / _TILE / _INST / _PAIR, *byte_offset and *bit as blsw_compact_locate.
 * The inverse of the placement of the four regions; the one statement of the rule: the device checker evaluates the same function.
 * BLSW_ERR_ARG: a NULL pointer, k or instance out of range, a struct that is not exactly what blsw_compact_layout_multi gives for some engine shape:
 * n is bounded on its own (n <= 65535 / n_pairs) before any product with it is formed, so no 64-bit product wraps, and every derived address is
 * proved inside [0, total) before it is used. Host only. */
int blsw_compact_locate_multi(const blsw_compact_layout_multi_t* layout, uint32_t k, uint64_t instance, uint32_t* region, uint64_t* byte_offset, uint32_t* bit);
/* blsw_compact_locate_multi of witnesses [k_begin, k_begin + count) of one instance: regions [count] u8, byte_offsets [count] u64, bits [count] u8. Host only. */
int blsw_compact_locate_multi_range(const blsw_compact_layout_multi_t* layout, uint32_t k_begin, uint32_t count, uint64_t instance, uint8_t* regions,
                                    uint64_t* byte_offsets, uint8_t* bits);
/* Pair families of a constraint system under such a layout: runs of K consecutive blocks of R rows in which block j reads nothing but column 0 and
 * witnesses of pair j (bit words and pair tiles) and equals block 0 entry for entry, every witness column moved by j strides of its run and every
 * coefficient identical. The checker evaluates ONE template block per family with one pair per lane. Nothing is assumed of the matrices: every entry
 * of every block is compared, and a system without such blocks has no family (the check then reads every row through the general path).
 * first_row / rows_per_pair [capacity] (may be NULL with capacity 0) receive the families in row order; *count = their number, also when it exceeds
 * capacity. BLSW_ERR_ARG: a NULL pointer, a CSR blsw_r1cs_create refuses, an inconsistent layout, layout->n_witness != info->n_witness.
 * Host only. blsw_r1cs_handle_pair_families answers the same for the matrices a handle was created from. The handle keeps no CSR: the first call
 * for a given K, set of runs and strides (the step size n does not enter) copies row pointers and entries back from the device with blocking
 * hipMemcpy calls — it synchronises the device, must not be made while a stream capture is in progress, and takes host time (1 s at K = 16) —
 * and the result stays on the handle; call it once before capturing or timing checks. This cache is the only state of a handle that a check,
 * an evaluation or this call changes; it is guarded by a mutex, so calls on one handle from several threads remain safe. */
int blsw_r1cs_pair_families(const blsw_matrices_info_t* info, const blsw_matrices_t* m, const blsw_compact_layout_multi_t* layout, uint64_t capacity,
                            uint64_t* first_row, uint64_t* rows_per_pair, uint64_t* count);
int blsw_r1cs_handle_pair_families(blsw_r1cs_t* r, const blsw_compact_layout_multi_t* layout, uint64_t capacity, uint64_t* first_row, uint64_t* rows_per_pair,
                                   uint64_t* count);
/* blsw_r1cs_check_compact / _evaluate_compact for a step of the N+1-pair product: n = layout->n instances (any legal step size, 4 and 32 included),
 * outputs [n], rows numbered as in the matrix, Montgomery form, d_instance as there. The check evaluates every pair family with one pair per lane
 * (whole tile rows, the template's entries read once instead of K times) and every other row with one instance per lane; the evaluation takes the
 * general path for any row window. d_first_unreduced: the instance vector, then every staged element of the three row regions at its index of z.
 * blsw_r1cs_check_compact_multi_ex is the same call with one more argument and is a public, supported symbol: use_families 1 is
 * blsw_r1cs_check_compact_multi; use_families 0 sends every row through the general path (same results; it needs no families and therefore never
 * reads the encoding back: the route for a caller inside a stream capture who has not called blsw_r1cs_handle_pair_families first, and the
 * yardstick of tools/r1cs_rate.py --multi); a value above 1 is BLSW_ERR_ARG. The first check with families per (handle, K, runs) computes them
 * as blsw_r1cs_handle_pair_families does, with its blocking copies. BLSW_ERR_ARG before any launch, nothing written: the rules
 * of blsw_r1cs_check_compact with the layout rules of blsw_compact_locate_multi. */
int blsw_r1cs_check_compact_multi(blsw_r1cs_t* r, const blsw_compact_layout_multi_t* layout, const void* d_compact, const uint64_t* d_instance,
                                  uint64_t instance_stride, int64_t* d_first_unsatisfied, int64_t* d_first_unreduced, void* stream);
int blsw_r1cs_check_compact_multi_ex(blsw_r1cs_t* r, const blsw_compact_layout_multi_t* layout, const void* d_compact, const uint64_t* d_instance,
                                     uint64_t instance_stride, uint32_t use_families, int64_t* d_first_unsatisfied, int64_t* d_first_unreduced, void* stream);
int blsw_r1cs_evaluate_compact_multi(blsw_r1cs_t* r, const blsw_compact_layout_multi_t* layout, const void* d_compact, const uint64_t* d_instance,
                                     uint64_t instance_stride, uint64_t row_begin, uint64_t row_count, uint64_t* d_az, uint64_t* d_bz, uint64_t* d_cz,
                                     void* stream);

/* Input decode (PublicKey::try_from / Signature::try_from -> deserialize_compressed, src/bls.rs:219-242, 316-339):
 *   d_pk48 [n][48], d_sig96 [n][96]  ZCash-format compressed points
 *   d_pk_xy [n][12], d_sig_xy [n][24] affine Montgomery coordinates in the layout blsw_engine_submit takes (identity / failure = zeros)
 *   d_status [n][2] int32: BLSW_ST_* of the key and of the signature (flags, x < p, on curve, prime-order subgroup;
 *   BLSW_ST_IDENTITY = well-formed encoding of the point at infinity)
 * tests/tests.rs:244-263 semantics: an instance verifies iff both statuses are BLSW_ST_OK and the gadget result is 1. */
int blsw_decode_batch(const uint8_t* d_pk48, const uint8_t* d_sig96, uint64_t n, uint64_t* d_pk_xy, uint64_t* d_sig_xy, int32_t* d_status, void* stream);

/* Signature::aggregate / PublicKey::aggregate (src/bls.rs:288-300, 183-195; tests/tests.rs:270-294 and the key sums of :296-334) for n
 * independent lists of k compressed points each: group 2 = signatures (G2, 96 bytes), group 1 = public keys (G1, 48 bytes).
 *   d_in [n][k][96 or 48]   d_out [n][96 or 48] the compressed sum (the infinity encoding for a sum that is the identity)
 *   d_status [n] int32: BLSW_ST_OK, or the status of the first point of the list that does not decode (try_from fails there: the
 *   reference unwraps); a well-formed point at infinity is a valid summand, as in aggregate_infinity_signature.json
 * An empty list is None in the reference: k == 0 is BLSW_ERR_ARG. Every point is decoded with its subgroup check by one lane, then one
 * lane per list adds. Asynchronous on `stream`; the workspace holds the decoded points. */
int blsw_aggregate_points_workspace_bytes(uint32_t group, uint64_t n, uint32_t k, uint64_t* bytes);
int blsw_aggregate_points_batch(uint32_t group, const uint8_t* d_in, uint32_t k, uint64_t n, uint8_t* d_out, int32_t* d_status, void* d_workspace,
                                uint64_t workspace_bytes, void* stream);

/* Weighted point sums and threshold recovery: d_out[i] = compressed sum_{j < count_i} s_ij * P_ij for n lists of k (point, scalar) terms with
 * caller-chosen full-size scalars, group 1 = public keys (G1, 48 bytes), group 2 = signatures (G2, 96 bytes) as in blsw_aggregate_points_batch.
 * This is the recombination of partial signatures or share keys with Lagrange coefficients, and the check of a share key against Feldman
 * commitments (pk_j == sum_i id_j^i C_i).
 *   blsw_combine_points_batch  d_in [n][k][48 | 96] compressed points, d_scalars32_le [n][k][32] little-endian scalars below r (zero is legal),
 *                              d_counts [n] (nullable: every list uses all k terms): list i uses its FIRST d_counts[i] terms; the terms behind
 *                              have no influence, whatever their bytes. d_term_status [n][k][2] int32 (nullable): the decode status of every
 *                              term's point and of its scalar, used or not.
 *   blsw_lagrange_batch        d_ids32_le [n][k][32] little-endian elements of Fr -> d_coeff32_le [n][k][32]:
 *                              lambda_j = prod_{m != j} id_m / prod_{m != j} (id_m - id_j) over the used ids — interpolation at 0; one id gives 1.
 *                              Rows j >= count_i are zeros, and every row of a failing list is zeros.
 *   blsw_recover_points_batch  the same sum with s_ij = lambda_ij(ids): the coefficients go into the workspace, then the combine stages run.
 * d_status [n] int32, in the order blsw_verify_pairs_batch uses for counts, then the terms:
 *     1. BLSW_ST_BAD_INDEX if count_i > k;
 *     2. else BLSW_ST_IDENTITY if count_i == 0;
 *     3. (recover and lagrange) else BLSW_ST_BAD_ENCODING for a used id >= r;
 *     4. (recover and lagrange) else BLSW_ST_BAD_ID for a used id that is zero or equal to another used id;
 *     5. (combine and recover) else the status of the lowest-indexed used term that is bad, the point's decode status before the scalar's
 *        (a scalar >= r is BLSW_ST_BAD_ENCODING). A well-formed identity point is a VALID term, as it is a valid summand of
 *        blsw_aggregate_points_batch, and so is a zero scalar;
 *     6. else BLSW_ST_OK.
 *   A failing list writes zeros to d_out[i]; a sum that is the identity writes the infinity encoding with BLSW_ST_OK — blsw_aggregate_points_batch's rule.
 * BLSW_ERR_ARG before any HIP call, nothing written: a group other than 1 or 2, n == 0, k == 0 or > 65535, n * k > 0x3fffffff, a NULL among the
 *   pointers not marked nullable. BLSW_ERR_WORKSPACE for a workspace below blsw_combine_points_workspace_bytes(group, n, k), which is
 *   non-decreasing in n and in k and serves blsw_recover_points_batch as well (the coefficients are part of it).
 * Workspace per term: G1 276 bytes (the decoded point 96, its status 4, the scaled Jacobian point 144, a coefficient 32); G2 4 836 bytes
 *   (192, 4, 4 608 = the scaled point and the 15 parked Jacobian points of the ladder's table, as the signer parks them, 32); 4 bytes per list.
 * Stages: blsw_aggregate_points_batch's decode lanes unchanged; one lane per list for the status; one lane per term for s * P — G2 by the
 *   signer's four-digit ladder, G1 by a two-digit ladder over (x, y) -> (beta x, y) with 128 doublings in place of 255; one lane per list for the
 *   sum, one inversion and the encoding. blsw_lagrange_batch: one lane per (list, j) with one inversion mod r, then one lane per list.
 * Measured (tools/combine_rate.py, profiles/combine_rate.txt; 65 536 terms in lists of 4 / 16 / 128, medians of five): G2 15.5 / 16.5 / 24.7 ms
 *   against blsw_sign_batch on 65 536 messages 16.7 / 17.2 / 18.2 ms; G1 7.0 / 7.3 / 10.0 ms against 10.4 / 10.6 / 14.0 ms with the plain 255-step
 *   ladder. The G1 table {P, Q, P + Q} is affine (one inversion per term): with P + Q Jacobian the lanes of a wavefront walked two addition
 *   bodies per step and the ladder was 1.05 x the plain one. The scale kernels run two waves per SIMD like the signer's; one wave, unspilled,
 *   measured the same (6.9 / 7.1 / 10.1 ms in G1). Recovery is 1.01 - 1.04 x the combine call up to 16 terms, 1.14 x at 128 in G1. Lists of 128
 *   terms pay a serial sum on one lane per list, as blsw_aggregate_points_batch does.
 * All four entries are fully asynchronous on `stream`: no synchronising copy, no allocation, no event wait — they need no hash stage and hence
 *   no step descriptor, so their arguments travel as kernel arguments, like blsw_aggregate_points_batch's.
 * PUBLIC SCALARS ONLY: the ladders branch on the scalar's bits and on the ids, as the signer's do on the key. Shares of a secret and the secret's
 *   recovery do not belong here. */
int blsw_combine_points_workspace_bytes(uint32_t group, uint64_t n, uint32_t k, uint64_t* bytes);
int blsw_combine_points_batch(uint32_t group, const uint8_t* d_in, const uint8_t* d_scalars32_le, const uint32_t* d_counts, uint32_t k, uint64_t n,
                              uint8_t* d_out, int32_t* d_status, int32_t* d_term_status, void* d_workspace, uint64_t workspace_bytes, void* stream);
int blsw_lagrange_batch(const uint8_t* d_ids32_le, const uint32_t* d_counts, uint32_t k, uint64_t n, uint8_t* d_coeff32_le, int32_t* d_status, void* stream);
int blsw_recover_points_batch(uint32_t group, const uint8_t* d_in, const uint8_t* d_ids32_le, const uint32_t* d_counts, uint32_t k, uint64_t n,
                              uint8_t* d_out, int32_t* d_status, void* d_workspace, uint64_t workspace_bytes, void* stream);

/* The same sum for LONG lists, by the bucket method (csrc/vmsm.hpp). New symbols only: the ABI number stays 17.
 *   blsw_msm_points_batch has blsw_combine_points_batch's contract word for word: d_in, d_scalars32_le, d_counts (nullable), group 1 / 2, the
 *   six-step status order, zeros for a failing list, the infinity encoding with BLSW_ST_OK for an identity sum, a well-formed identity point and a
 *   zero scalar as valid terms. For every input both entries accept, d_out and d_status are byte for byte what blsw_combine_points_batch writes.
 *   There is no d_term_status. k may go up to 2^24 (16 777 216); n * k <= 0x3fffffff still holds.
 *   window_bits: 0 = the library's choice from k (csrc/vmsm.hpp: msm_default_window); 1 .. 16 are taken as given (tuning, and tests reach every
 *   path at small k with it).
 * BLSW_ERR_ARG before any HIP call, nothing written: a group other than 1 or 2, n == 0, k == 0 or > 2^24, n * k > 0x3fffffff, window_bits > 16, a
 *   NULL among the pointers not marked nullable. BLSW_ERR_WORKSPACE for a workspace below blsw_msm_workspace_bytes(group, n, k, window_bits),
 *   which is non-decreasing in n and in k for a fixed window_bits (0 included).
 * Workspace with c = window bits, W = ceil(255 / c), B = 2^c: per term the decoded point and its status (G1 100, G2 196 bytes) and 4 W bytes of
 *   sorted indices; per list 8 W B bytes of counts and cursors and W (B + ceil(B / 32) + 1) Jacobian points of 144 (G1) or 288 (G2) bytes.
 * Stages: blsw_aggregate_points_batch's decode lanes and the combine entry's status rule unchanged; one lane per term counts its non-zero c-bit
 *   digits into a histogram per (list, window); a prefix scan; one lane per term scatters its index into bucket order through an atomic cursor;
 *   one lane per (list, window, bucket) adds its bucket's points; one lane per 32 buckets and then one per (list, window) form sum_b b B_b; one lane
 *   per list combines the windows, inverts once and encodes. The order inside a bucket is not fixed; every addition is the complete four-branch
 *   form, so the sum — a group element — and its bytes are.
 * Measured (tools/msm_rate.py, profiles/msm_rate.txt; MI355X, ONE list, medians of five, the existing path in the same run): 65 536 terms G1
 *   48 ms, G2 92 ms, blsw_registry_msm_batch 66 ms, against blsw_combine_points_batch on 65 535 + 1 terms and blsw_aggregate_points_batch
 *   1 725 ms and 4 914 ms (spreads 436 and 1 351 ms); 2^20 terms 0.50 s, 0.64 s and 0.96 s against 2.0 s and 5.4 s. Half of the call at 65 536
 *   terms and four fifths at 2^20 is the status rule, which walks the list on one lane (profiles/msm_stages.txt).
 * One long bucket: when all scalars are equal, one bucket per window takes every term and one lane adds them one after the other. The result is
 *   right; the time is that of k serial mixed additions and is not hidden — measured at 65 536 equal scalars: G1 1.46 s, G2 4.48 s, about what
 *   the combine entry's one-lane sum takes. Long buckets are not split. A window of 2 or 3 bits is the same effect (4 .. 8 buckets share all
 *   terms): with c = 7, 9, 11, 12 or 14 the top window is that narrow (65 536 terms, G1: 219 .. 360 ms instead of 48), so the library's choice is
 *   among 5, 8, 13 and 15.
 * Which entry: blsw_combine_points_batch pays a ladder per term and sums a list on one lane, this entry pays about W mixed additions per term and
 *   a fixed tail of a few hundred additions per list. Measured on one list, the per-term ladder wins up to 64 terms (G1 8.0 against 8.4 ms, G2
 *   17.6 against 21.8 ms) and the buckets from 256 terms on (9.8 against 12.7 ms, 22.0 against 32.6 ms; 3.6 x at 1 024, 10 x at 4 096): the
 *   crossover lies between 64 and 256 terms of ONE list. Many short lists fill the device with ladders and belong there.
 * Fully asynchronous on `stream`: no synchronising copy, no allocation, no event wait. PUBLIC SCALARS ONLY: the digits and the bucket indices
 *   depend on the scalars. */
int blsw_msm_workspace_bytes(uint32_t group, uint64_t n, uint32_t k, uint32_t window_bits, uint64_t* bytes);
int blsw_msm_points_batch(uint32_t group, const uint8_t* d_in, const uint8_t* d_scalars32_le, const uint32_t* d_counts, uint32_t k, uint64_t n,
                          uint32_t window_bits, uint8_t* d_out, int32_t* d_status, void* d_workspace, uint64_t workspace_bytes, void* stream);

/* hash_to_g2 only(src/hasher.rs:727-740 / src/bls.rs:477-493): d_out_affine [n][24] u64 (x.c0, x.c1, y.c0, y.c1) Montgomery */
int blsw_hash_to_g2_workspace_bytes(uint64_t n, uint32_t msg_len, uint64_t* bytes);
int blsw_hash_to_g2_batch(const uint8_t* d_msg, uint32_t msg_len, uint64_t n, uint64_t* d_out_affine, void* d_workspace, uint64_t workspace_bytes,
                          void* stream);

/* Native signer for a batch: BLS::sign (src/bls.rs:411-425: sig = sk * H(msg); Err(InvalidSecretKey) for sk = 0) and
 * PublicKey::from(&sk) (src/bls.rs:183-195: pk = sk * g1). One key per instance.
 *   d_sk32_le [n][32]  secret keys as PrivateKey::try_from(&[u8]) takes them (src/bls.rs:97-103): little-endian Fr
 *   outputs, each nullable except d_status: d_sig96 [n][96] / d_pk48 [n][48] compressed points as Signature / PublicKey
 *   serialise (src/bls.rs:244-260, 341-357), d_sig_xy [n][24] / d_pk_xy [n][12] affine Montgomery limbs (engine input)
 *   d_status [n] int32: BLSW_ST_OK, BLSW_ST_BAD_ENCODING (sk >= r) or BLSW_ST_INVALID_SECRET_KEY (sk = 0); on error
 *   the outputs of that instance are the identity encoding / zeros.
 * Workspace: blsw_hash_to_g2_workspace_bytes(n, msg_len). */
int blsw_sign_batch(const uint8_t* d_sk32_le, const uint8_t* d_msg, uint32_t msg_len, uint64_t n, uint8_t* d_sig96, uint64_t* d_sig_xy, uint8_t* d_pk48,
                    uint64_t* d_pk_xy, int32_t* d_status, void* d_workspace, uint64_t workspace_bytes, void* stream);

/* BLS::verify (src/bls.rs:427-458; tests/tests.rs:239-268) for a batch, as VALUES — the native algorithm, not the circuit: decode of the compressed key and
 * signature with the endomorphism subgroup checks (as blsw_decode_batch), hash_to_g2 (as blsw_hash_to_g2_batch), a two-pair Miller loop over projective
 * line coefficients (no inversion per step) and the final exponentiation on six lanes per instance, is_one.
 *   d_pk48 [n][48], d_sig96 [n][96], d_msg [n][msg_len];  d_result [n] int32: 1 iff both points decode to non-identity points of the prime-order
 *   subgroups and e(-g1, sig) * e(pk, H(msg)) == 1 (every Err of the reference's verify counts as false, as tests/tests.rs:244-263 does);
 *   d_status [n][2] BLSW_ST_* of key and signature. Asynchronous on `stream` after one synchronising descriptor copy. fast_aggregate_verify
 *   (tests/tests.rs:296-334) = blsw_aggregate_points_batch over the keys, then this. */
int blsw_verify_workspace_bytes(uint64_t n, uint32_t msg_len, uint64_t* bytes);
int blsw_verify_batch(const uint8_t* d_pk48, const uint8_t* d_sig96, const uint8_t* d_msg, uint32_t msg_len, uint64_t n, int32_t* d_result, int32_t* d_status,
                      void* d_workspace, uint64_t workspace_bytes, void* stream);

/* ABI 17: batch verification of GROUPS of triples with random coefficients, the form every consensus client verifies in (blst's
 * verify_multiple_aggregate_signatures). Group j is instances [j * group, min(n, (j + 1) * group)): ceil(n / group) groups, the last one may be short,
 * group > n gives one group. With the caller's 64-bit coefficients r_i = d_scalars[i]
 *     d_group_result[j] = 1  iff  every instance of the group has both statuses BLSW_ST_OK and r_i != 0,  and
 *                                 prod_i e(r_i pk_i, H(msg_i)) * e(-g1, sum_i r_i sig_i) == 1
 * — one final exponentiation per group, one line chain per instance, and the squarings of the Miller loop shared by the BLSW_VGROUP_CHUNK pairs one
 * six-lane team folds. It fails closed: a zero coefficient makes its group 0; an instance whose status is not OK contributes nothing to the product or
 * the sum (its points are zeros) and makes its group 0. d_status [n][2] is exactly what blsw_verify_batch writes. The library reads no entropy, as it
 * reads no environment: the coefficients are the caller's. What callers (and the tests) can rest on:
 *   P1  all instances of a group valid                              -> 1 for ANY non-zero coefficients.
 *   P2  exactly one instance fails its pairing equation, all statuses OK, all coefficients non-zero
 *                                                                   -> 0 for ANY such coefficients: GT has prime order r > 2^64, so e_bad^(r_bad) != 1.
 *   P3  group == 1                                                  -> the verdict of blsw_verify_batch, for any non-zero coefficient.
 *   P4  two or more invalid instances: the group passes only if the coefficients satisfy one linear relation mod r. Independent, uniform,
 *       unpredictable 64-bit coefficients chosen AFTER the inputs are fixed accept a bad group with probability <= 2^-64.
 * The subgroup checks of the decode are what make this sound: P2 and P4 argue in groups of prime order r, and a point outside them could carry a
 * small-order component that a coefficient kills. Predictable coefficients are not sound: with EQUAL coefficients the two invalid triples
 * (pk, m1, sig2) and (pk, m2, sig1), sig_k = sk * H(m_k), pass as a group — their signatures are swapped, and the sum does not see it.
 *   BLSW_ERR_ARG before any HIP call: group == 0 or > 65535, n == 0 or > 0x7fffffff, msg_len > 65535, a NULL among d_pk48, d_sig96, d_scalars,
 *   d_group_result, d_status, d_workspace, or d_msg == NULL with msg_len != 0. BLSW_ERR_WORKSPACE for a workspace below
 *   blsw_verify_groups_workspace_bytes(n, msg_len, group) — smaller than blsw_verify_workspace_bytes: it holds one set of lines, not two.
 *   Asynchronous on `stream` after one synchronising descriptor copy, as blsw_verify_batch. */
#ifndef BLSW_VGROUP_CHUNK
#define BLSW_VGROUP_CHUNK 8 /* pairs one six-lane team folds with shared squarings (<= 31). Provisional, not measured: at n = 65 536 it launches 8 192 teams, under the 10 240 resident at once */
#endif
int blsw_verify_groups_workspace_bytes(uint64_t n, uint32_t msg_len, uint32_t group, uint64_t* bytes);
int blsw_verify_groups_batch(const uint8_t* d_pk48, const uint8_t* d_sig96, const uint8_t* d_msg, uint32_t msg_len, uint64_t n, const uint64_t* d_scalars,
                             uint32_t group, int32_t* d_group_result, int32_t* d_status, void* d_workspace, uint64_t workspace_bytes, void* stream);

/* AggregateVerify of the BLS signature draft as VALUES: ONE aggregate signature over n_pairs (key, message) pairs with their own messages,
 *     e(-g1, sig) * prod_j e(pk_j, H(msg_j)) == 1
 * from compressed bytes — the third verification form next to blsw_verify_batch (Verify) and the fast_aggregate_verify entries. New symbols only: the
 * ABI number stays 17. Every key and the signature are decoded with their subgroup checks, every message is hashed to G2, every used pair gets one
 * projective line chain (no inversion per step), a six-lane team folds BLSW_VPAIRS_CHUNK pairs with shared squarings, and an instance pays ONE final
 * exponentiation (csrc/vpairs.hpp). The ciphersuite is the library's one (..._POP_): repeated messages are legal, no distinctness check is made.
 *   d_pks48 [n][n_pairs][48], d_msgs [n][n_pairs][msg_len], d_sig96 [n][96]
 *   d_counts [n] uint32 (nullable): instance i uses its FIRST count_i pairs — ragged lists travel padded to the longest; NULL = all n_pairs
 *   d_key_status [n][n_pairs] int32 (nullable): BLSW_ST_* of every key, used or not
 *   d_status [n][2] int32: [i][1] the signature's status exactly as blsw_verify_batch writes it; [i][0], in this order:
 *     1. BLSW_ST_BAD_INDEX if count_i > n_pairs: no verdict depends on anything the instance holds;
 *     2. else BLSW_ST_IDENTITY if count_i == 0 (the draft requires at least one pair; as the committee form's empty selection);
 *     3. else the status of the lowest-indexed USED pair whose key is not BLSW_ST_OK — a well-formed identity key is BLSW_ST_IDENTITY here: every
 *        key goes through KeyValidate, as BLS::verify rejects the identity key, and unlike a summand of PublicKey::aggregate;
 *     4. else BLSW_ST_OK.
 *   d_result [n] int32: 1 iff both entries of d_status[i] are BLSW_ST_OK and the product over the used pairs is one. Every error counts as false.
 * What callers (and the tests) can rest on:
 *   Q1  n_pairs == 1, d_counts == NULL: d_result and d_status are exactly blsw_verify_batch's.
 *   Q2  the verdict does not change under a permutation of an instance's used pairs; pairs at j >= count_i have no influence whatever their bytes.
 *   Q3  all used messages of an instance equal: the verdict of fast_aggregate_verify on the same keys (blsw_aggregate_points_batch(1, ..), then
 *       blsw_verify_batch) — except for a list with a well-formed identity key, which the aggregate form accepts as a summand and this one refuses.
 *   Q4  on non-identity points of the prime-order subgroups the verdict is the Boolean of the N+1-pair circuit (blsw_verify_multi_batch).
 * BLSW_ERR_ARG before any HIP call, nothing written: n == 0, n_pairs == 0 or > 65535, n * n_pairs > 0x7fffffff, msg_len > 65535, a NULL among
 *   d_pks48, d_sig96, d_result, d_status, d_workspace, or d_msgs == NULL with msg_len != 0. BLSW_ERR_WORKSPACE for a workspace below
 *   blsw_verify_pairs_workspace_bytes(n, msg_len, n_pairs), which is non-decreasing in each argument. What this entry adds to it is dominated by ONE
 *   set of lines per pair, BLSW_VLINE_ROWS (6 * 68 field elements) * 48 bytes = 19.6 KB (n * n_pairs = 65 536 pairs: 1.3 GB); the hash's carve that
 *   every value entry shares stands next to it with 109 KB per message (without the buffers of the latency kernels, which blsw_verify_batch's
 *   workspace carries up to 4 096 instances): about 130 KB per pair in all, by which callers size their calls.
 *   Asynchronous on `stream` after the one synchronising descriptor copy the other value entries make. */
#ifndef BLSW_VPAIRS_CHUNK
#define BLSW_VPAIRS_CHUNK 8 /* pairs one six-lane team folds with shared squarings (<= 31). Measured at K = 128, n = 512 (65 536 pairs; profiles/pairs_rate.txt): 2 -> 61.6, 4 -> 54.9, 8 -> 51.3, 16 -> 64.4, 31 -> 87.4 ms: from 16 on the call has fewer teams (4 096) than the device holds at once (10 240) */
#endif
int blsw_verify_pairs_workspace_bytes(uint64_t n, uint32_t msg_len, uint32_t n_pairs, uint64_t* bytes);
int blsw_verify_pairs_batch(const uint8_t* d_pks48, const uint8_t* d_msgs, uint32_t msg_len, uint32_t n_pairs, const uint32_t* d_counts, const uint8_t* d_sig96,
                            uint64_t n, int32_t* d_result, int32_t* d_status, int32_t* d_key_status, void* d_workspace, uint64_t workspace_bytes, void* stream);

/* fast_aggregate_verify (tests/tests.rs:296-334) as VALUES over ONE committee and many bitmaps, the shape of a sync-committee verifier: K keys
 * given once, and per instance a participation bitmap, one message and one aggregate signature. New symbols only: the ABI number stays 17. The
 * committee is decoded ONCE per call (K subgroup checks, not n * K), every instance sums its selected keys with BLSW_COMMITTEE_LANES lanes (a
 * mixed addition per selected key and lane, then a log2 tree of general additions; csrc/committee.hpp), and the aggregated keys go to the two
 * verifiers above unchanged.
 *   d_pks48 [n_keys][48]  the committee, compressed          d_bitmap [n][n_keys] bytes, a non-zero byte selects the key
 *   d_sig96 [n][96], d_msg [n][msg_len]
 *   d_key_status [n_keys] int32: BLSW_ST_* of every committee key, written whether or not any instance selects it
 *   d_count [n] uint32 (nullable): the number of selected keys, the `count` of aggregate_verify
 *   d_agg48 [n][48] (nullable): the compressed sum of the selected keys (the infinity encoding for the identity, an empty selection included;
 *     zeros when a selected key does not decode) — byte for byte what blsw_aggregate_points_batch(1, ...) gives for the same keys in the same order
 *   d_status [n][2] int32: [i][1] the signature's status as blsw_verify_batch writes it; [i][0] the status of instance i's aggregate key:
 *     the status of the lowest-indexed SELECTED key that is neither OK nor IDENTITY if there is one, else BLSW_ST_IDENTITY if the sum is the
 *     identity (an empty selection included), else BLSW_ST_OK. A selected key that is the well-formed identity is a valid summand, as in
 *     PublicKey::aggregate (src/bls.rs:183-195): it adds nothing to the sum and is counted in d_count. A key that does not decode and is not
 *     selected has no effect on any instance.
 * group == 0, per instance: d_scalars must be NULL, d_result is [n]; d_result[i] is exactly the verdict of blsw_verify_batch on (d_agg48[i], msg_i,
 *   sig_i), 0 whenever d_status[i][0] is not OK — fast_aggregate_verify on the selected keys; an empty selection is false, as its k == 0.
 * group >= 1, grouped: d_scalars [n] is required, d_result is [ceil(n / group)]: exactly the statement of blsw_verify_groups_batch and its
 *   properties P1-P4 with pk_i = the aggregate of instance i and its status = d_status[i][0]; an instance whose aggregate status is not OK is
 *   excluded and fails its group, as there.
 * BLSW_ERR_ARG before any HIP call, nothing written: n_keys == 0 or > 65535, n == 0 or > 0x7fffffff, msg_len > 65535, group > 65535, a NULL among
 *   d_pks48, d_bitmap, d_sig96, d_result, d_status, d_key_status, d_workspace, d_scalars non-NULL with group == 0 or NULL with group >= 1, or
 *   d_msg == NULL with msg_len != 0. BLSW_ERR_WORKSPACE for a workspace below blsw_committee_verify_workspace_bytes(n, msg_len, n_keys, group): it
 *   holds what the chosen verifier's workspace holds, the decoded committee ([2][n_keys] field elements, read n times and meant to stay in cache)
 *   and the hash's carve. Asynchronous on `stream` after the one synchronising descriptor copy the two verifiers make.
 * There is no committee handle, on purpose: decoding K keys is K lanes in the launch that also decodes the n signatures, so a per-call decode costs no
 * extra latency, and a handle would only add lifetime rules. */
#ifndef BLSW_COMMITTEE_LANES
#define BLSW_COMMITTEE_LANES 16 /* lanes that share one instance's sum; a power of two <= 64. Measured at K = 512, n = 8 192 (profiles/committee_rate.txt): 4, 8, 16, 32, 64 lanes lie within 4 % of each other, 16 lowest */
#endif
int blsw_committee_verify_workspace_bytes(uint64_t n, uint32_t msg_len, uint32_t n_keys, uint32_t group, uint64_t* bytes);
int blsw_committee_verify_batch(const uint8_t* d_pks48, uint32_t n_keys, const uint8_t* d_bitmap, const uint8_t* d_sig96, const uint8_t* d_msg,
                                uint32_t msg_len, uint64_t n, const uint64_t* d_scalars, uint32_t group, int32_t* d_result, uint32_t* d_count,
                                int32_t* d_status, int32_t* d_key_status, uint8_t* d_agg48, void* d_workspace, uint64_t workspace_bytes, void* stream);

/* fast_aggregate_verify as VALUES over a RESIDENT registry of keys and n INDEX LISTS, the shape of a consensus client's signature sets: (a list of
 * validator indices, one message, one aggregate signature) over 10^5 .. 10^6 keys that change only by appending. New symbols only: the ABI number
 * stays 17. A committee of that size cannot be decoded inside the call (and a bitmap row per set would be n * K bytes), so the keys get a handle:
 * they are decoded ONCE, when appended, into 128-byte records (x, y, status: one cache line per gathered key; csrc/registry.hpp) that stay in the
 * caller's device buffer, and a call sums each list's records with BLSW_REGISTRY_LANES lanes and hands the sums to the two verifiers above unchanged.
 * The handle follows the conventions of blsw_keyset_create: the caller owns d_buffer (256-byte aligned, blsw_registry_bytes(capacity) bytes), which
 * must outlive the handle and every call that names it; device -1 = the current device; every rule is checked on the host before any HIP call.
 *   blsw_registry_create: an empty registry of room for `capacity` keys, 1 .. 2^24 (16 777 216). Nothing is launched; the buffer is not cleared.
 *   blsw_registry_append: d_pks48 [count][48] compressed keys become keys [size, size + count): decoded with the subgroup check, one lane per key,
 *     asynchronously on `stream`. size grows ON THE HOST AT THE CALL. BLSW_ERR_ARG: a NULL handle or d_pks48, count == 0, size + count > capacity.
 *   blsw_registry_size: the number of keys appended so far.
 *   blsw_registry_key_status: the device array [capacity] int32 of the keys' BLSW_ST_*; entries [0, size) are defined once their appends have run.
 *   blsw_registry_destroy: frees the handle; the buffer is the caller's.
 * A verify call must be ORDERED BEHIND the appends it relies on (the same stream, or an event): it reads records the appends write. The handle is
 * NOT thread-safe: append, size and verify calls on one handle must not run concurrently.
 *   blsw_registry_verify_batch: set i is d_indices[d_offsets[i] .. d_offsets[i + 1]) — CSR, d_offsets [n + 1] uint64, d_indices [n_indices] uint32.
 *   d_sig96 [n][96], d_msg [n][msg_len]; d_status [n][2] int32: [i][1] the signature's status as blsw_verify_batch writes it; [i][0], in this order:
 *     1. BLSW_ST_BAD_INDEX if d_offsets[i] > d_offsets[i + 1] or d_offsets[i + 1] > n_indices (or the list is longer than 2^32 - 2 entries): no
 *        entry of the set is read;
 *     2. else the status of the EARLIEST LIST POSITION whose entry is bad — an index >= size as of the call is BLSW_ST_BAD_INDEX (also one below
 *        capacity that is not yet appended: its row is never read, so no stale row can count), a key whose status is neither OK nor IDENTITY
 *        gives that status;
 *     3. else BLSW_ST_IDENTITY if the sum is the identity (the empty list included);  4. else BLSW_ST_OK.
 *     A repeated index is added as often as it occurs; a selected identity key is a valid summand (PublicKey::aggregate, src/bls.rs:183-195).
 *   d_agg48 [n][48] (nullable): byte for byte what blsw_aggregate_points_batch(1, ...) gives for the gathered keys in list order (the infinity
 *     encoding for the identity and the empty list); zeros when the set has a bad entry or bad offsets.
 *   group == 0 / group >= 1, d_scalars and the length of d_result: word for word as blsw_committee_verify_batch — per set the verdict of
 *     blsw_verify_batch on (d_agg48[i], msg_i, sig_i), 0 whenever d_status[i][0] is not OK; or blsw_verify_groups_batch's statement and its
 *     properties P1-P4 with pk_i = the set's sum and its status = d_status[i][0].
 * BLSW_ERR_ARG before any HIP call, nothing written: n == 0 or > 0x7fffffff, msg_len > 65535, group > 65535, a NULL among r, d_offsets, d_sig96,
 *   d_result, d_status, d_workspace, d_scalars non-NULL with group == 0 or NULL with group >= 1, d_msg == NULL with msg_len != 0, d_indices == NULL
 *   with n_indices != 0, n_indices > 2^40, a registry of size 0. BLSW_ERR_WORKSPACE for a workspace below
 *   blsw_registry_verify_workspace_bytes(n, msg_len, group): what the chosen verifier's workspace holds and the hash's carve — no table, it lives in
 *   the handle. Asynchronous on `stream` (a stream of the handle's device) after the one synchronising descriptor copy the two verifiers make. */
#ifndef BLSW_REGISTRY_LANES
#define BLSW_REGISTRY_LANES 16 /* lanes that share one set's sum; a power of two <= 64. Measured (profiles/registry_rate.txt): at K = 512, n = 8 192 16 is lowest (4 .. 64 within 3 %); at 2^20 keys, n = 2 048 sets of 400 - 500 and 1 indices 32 is lowest and 16 lies 0.5 % above it */
#endif
typedef struct blsw_registry blsw_registry_t;
int blsw_registry_bytes(uint32_t capacity, uint64_t* bytes);
int blsw_registry_create(blsw_registry_t** out, uint32_t capacity, int32_t device, void* d_buffer, uint64_t buffer_bytes);
int blsw_registry_append(blsw_registry_t* r, const uint8_t* d_pks48, uint32_t count, void* stream);
int blsw_registry_size(const blsw_registry_t* r, uint32_t* n_keys);
int blsw_registry_key_status(const blsw_registry_t* r, const int32_t** d_status); /* [capacity], entries [0, size) defined */
int blsw_registry_destroy(blsw_registry_t* r);
int blsw_registry_verify_workspace_bytes(uint64_t n, uint32_t msg_len, uint32_t group, uint64_t* bytes);
int blsw_registry_verify_batch(const blsw_registry_t* r, const uint32_t* d_indices, uint64_t n_indices, const uint64_t* d_offsets, const uint8_t* d_sig96,
                               const uint8_t* d_msg, uint32_t msg_len, uint64_t n, const uint64_t* d_scalars, uint32_t group, int32_t* d_result, int32_t* d_status,
                               uint8_t* d_agg48, void* d_workspace, uint64_t workspace_bytes, void* stream);
/* sum_p s_p * key[index_p] over index lists of a registry, by the bucket method of blsw_msm_points_batch (G1 only; new symbols, ABI 17): list i is
 * d_indices[d_offsets[i] .. d_offsets[i + 1]) in CSR form as above, position p of d_indices carries the scalar d_scalars32_le[p] (32 little-endian
 * bytes below r, PUBLIC). No key is decoded: the records are read as they stand. d_status [n] int32, in this order:
 *     1. BLSW_ST_BAD_INDEX for bad offsets, by rule 1 above: no entry of the list is read;
 *     2. else BLSW_ST_IDENTITY for an empty list (the combine rule);
 *     3. else the status of the EARLIEST LIST POSITION that is bad; within a position: an index >= size as of the call is BLSW_ST_BAD_INDEX and its
 *        record is never read; a key whose status is neither OK nor IDENTITY gives that status; a scalar >= r is BLSW_ST_BAD_ENCODING;
 *     4. else BLSW_ST_OK.
 *   A repeated index counts as often as it occurs; an identity key and a zero scalar are valid terms. d_out48 [n][48]: zeros for a failing list,
 *   the infinity encoding for an identity sum; for an OK list the bytes blsw_combine_points_batch gives on the gathered keys.
 *   window_bits as in blsw_msm_points_batch; 0 chooses by the MEAN list length n_indices / n.
 * BLSW_ERR_ARG before any HIP call, nothing written: n == 0 or > 0x7fffffff, a NULL among r, d_offsets, d_out48, d_status, d_workspace,
 *   d_indices or d_scalars32_le NULL with n_indices != 0, n_indices > 2^40, a registry of size 0, window_bits > 16. BLSW_ERR_WORKSPACE below
 *   blsw_registry_msm_workspace_bytes(n, n_indices, window_bits): non-decreasing in n and in n_indices for window_bits 1 .. 16, and in n_indices
 *   for window_bits 0 (there more lists over the same indices are shorter lists and may get narrower windows).
 * Lists that are valid one by one can share positions when a bad list lies between them (offsets 0, 5, 3, 8); such lists are summed by one lane
 *   each with the per-term ladder — the same bytes, the combine entry's speed. The status lane walks its list once, one lane per list.
 * Must be ordered behind the appends it relies on, like the verify call. Fully asynchronous on `stream`. */
int blsw_registry_msm_workspace_bytes(uint64_t n, uint64_t n_indices, uint32_t window_bits, uint64_t* bytes);
int blsw_registry_msm_batch(const blsw_registry_t* r, const uint32_t* d_indices, uint64_t n_indices, const uint64_t* d_offsets, const uint8_t* d_scalars32_le,
                            uint64_t n, uint32_t window_bits, uint8_t* d_out48, int32_t* d_status, void* d_workspace, uint64_t workspace_bytes, void* stream);

/* A CALLER-CHOSEN DOMAIN SEPARATION TAG for the value entries, and PopProve / PopVerify. New symbols only: the ABI number stays 17 and
 * blsw_engine_options_t is untouched. Every entry above hashes under the library's tag, BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_; the *_dst
 * entries below take the tag of hash_to_curve (RFC 9380 5.3.1, expand_message_xmd with SHA-256) as an argument, so that the proof-of-possession tag
 * BLS_POP_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_ of the signature draft, the ..._NUL_ and ..._AUG_ suites' tags and application tags can be used.
 *   blsw_dst_t: the tag's bytes and its length, 1 .. 255. A tag of more than 255 bytes (RFC 9380 5.3.3 hashes it down first) is NOT offered.
 *   blsw_dst_set: BLSW_ERR_ARG for a NULL argument, len == 0 or len > 255 (BLSW_DST_MAX_LEN); bytes behind the tag are zeroed.
 *   blsw_dst_default / blsw_dst_pop: the library's tag / the BLS_POP_... tag (43 bytes each).
 * The tag travels to the device as a KERNEL ARGUMENT laid out on the host once per call (csrc/sha.hpp: DstArg), so every *_dst entry takes the
 * workspace of its plain form. `dst` == NULL is the plain entry exactly (the same kernels, the same bits); a non-NULL tag always runs the
 * tag-taking hash kernel, also when it equals the library's tag — the results are the same bits. A non-NULL tag of length 0 is BLSW_ERR_ARG.
 * Everything else — arguments, statuses, verdicts, properties, errors — is word for word the plain entry's. b_0 of a message hashes
 * ceil((77 + msg_len + len) / 64) blocks and each of the eight b_i ceil((43 + len) / 64): 1 block up to 21 tag bytes, 2 up to 85 (the library's
 * tag), 3 up to 149, 4 up to 213, 5 up to 255.
 * What stays out: the tag of the witness engine and the circuits (constant bits folded into the SHA gadget: another tag is another circuit);
 * tags beyond 255 bytes; messages of different lengths in one call; a registry that admits keys only with a proof of possession
 * (blsw_registry_append is unchanged: callers run blsw_pop_verify_batch first). */
#define BLSW_DST_MAX_LEN 255
typedef struct {
    uint8_t bytes[255];
    uint8_t len;
} blsw_dst_t;
int blsw_dst_set(blsw_dst_t* out, const uint8_t* tag, uint32_t len);
int blsw_dst_default(blsw_dst_t* out);
int blsw_dst_pop(blsw_dst_t* out);
/* hash_to_field of RFC 9380 5.2 for G2 (count 2, m 2, L 64) on its own: d_msg [n][msg_len] -> d_u [n][4][6] u64 Montgomery in the order u0.c0, u0.c1,
 * u1.c0, u1.c1 — the only thing the tag changes in any entry. No workspace, no descriptor copy: asynchronous on `stream`. dst == NULL = the
 * library's tag. BLSW_ERR_ARG: n == 0 or > 0x7fffffff, msg_len > 65535, d_u == NULL, d_msg == NULL with msg_len != 0, a tag of length 0. */
int blsw_hash_to_field_batch(const uint8_t* d_msg, uint32_t msg_len, uint64_t n, const blsw_dst_t* dst, uint64_t* d_u, void* stream);
int blsw_hash_to_g2_batch_dst(const uint8_t* d_msg, uint32_t msg_len, uint64_t n, uint64_t* d_out_affine, void* d_workspace, uint64_t workspace_bytes,
                              const blsw_dst_t* dst, void* stream);
int blsw_sign_batch_dst(const uint8_t* d_sk32_le, const uint8_t* d_msg, uint32_t msg_len, uint64_t n, uint8_t* d_sig96, uint64_t* d_sig_xy, uint8_t* d_pk48,
                        uint64_t* d_pk_xy, int32_t* d_status, void* d_workspace, uint64_t workspace_bytes, const blsw_dst_t* dst, void* stream);
int blsw_verify_batch_dst(const uint8_t* d_pk48, const uint8_t* d_sig96, const uint8_t* d_msg, uint32_t msg_len, uint64_t n, int32_t* d_result,
                          int32_t* d_status, void* d_workspace, uint64_t workspace_bytes, const blsw_dst_t* dst, void* stream);
int blsw_verify_groups_batch_dst(const uint8_t* d_pk48, const uint8_t* d_sig96, const uint8_t* d_msg, uint32_t msg_len, uint64_t n, const uint64_t* d_scalars,
                                 uint32_t group, int32_t* d_group_result, int32_t* d_status, void* d_workspace, uint64_t workspace_bytes,
                                 const blsw_dst_t* dst, void* stream);
int blsw_verify_pairs_batch_dst(const uint8_t* d_pks48, const uint8_t* d_msgs, uint32_t msg_len, uint32_t n_pairs, const uint32_t* d_counts,
                                const uint8_t* d_sig96, uint64_t n, int32_t* d_result, int32_t* d_status, int32_t* d_key_status, void* d_workspace,
                                uint64_t workspace_bytes, const blsw_dst_t* dst, void* stream);
int blsw_committee_verify_batch_dst(const uint8_t* d_pks48, uint32_t n_keys, const uint8_t* d_bitmap, const uint8_t* d_sig96, const uint8_t* d_msg,
                                    uint32_t msg_len, uint64_t n, const uint64_t* d_scalars, uint32_t group, int32_t* d_result, uint32_t* d_count,
                                    int32_t* d_status, int32_t* d_key_status, uint8_t* d_agg48, void* d_workspace, uint64_t workspace_bytes,
                                    const blsw_dst_t* dst, void* stream);
int blsw_registry_verify_batch_dst(const blsw_registry_t* r, const uint32_t* d_indices, uint64_t n_indices, const uint64_t* d_offsets, const uint8_t* d_sig96,
                                   const uint8_t* d_msg, uint32_t msg_len, uint64_t n, const uint64_t* d_scalars, uint32_t group, int32_t* d_result,
                                   int32_t* d_status, uint8_t* d_agg48, void* d_workspace, uint64_t workspace_bytes, const blsw_dst_t* dst, void* stream);
/* PopProve of the signature draft (POP ciphersuite) for a batch: pk_i = sk_i * g1 and proof_i = sk_i * H_pop(pk_i's 48 compressed bytes), H_pop =
 * hash_to_g2 under the BLS_POP_... tag.
 *   d_sk32_le [n][32] as blsw_sign_batch takes them; d_proof96 [n][96], d_pk48 [n][48] compressed, both REQUIRED (the key bytes are the proof's
 *   message); d_status [n] int32 exactly blsw_sign_batch's: BLSW_ST_OK, BLSW_ST_BAD_ENCODING (sk >= r) or BLSW_ST_INVALID_SECRET_KEY (sk = 0),
 *   and on error both outputs of the instance are the infinity encoding.
 * Workspace: blsw_hash_to_g2_workspace_bytes(n, 48). BLSW_ERR_ARG: n == 0 or > 0x7fffffff, a NULL pointer. */
int blsw_pop_prove_batch(const uint8_t* d_sk32_le, uint64_t n, uint8_t* d_proof96, uint8_t* d_pk48, int32_t* d_status, void* d_workspace,
                         uint64_t workspace_bytes, void* stream);
/* PopVerify for a batch: KeyValidate (the key decodes, lies in the prime-order subgroup and is not the identity), the proof decodes the same way, and
 * e(-g1, proof) * e(pk, H_pop(pk48)) == 1. It IS blsw_verify_batch_dst with the key bytes as the message and the BLS_POP_... tag: d_result [n],
 * d_status [n][2] (key, proof), arguments and errors as there. Workspace: blsw_verify_workspace_bytes(n, 48). A signature over the key bytes made
 * under the library's tag is refused: that is what the second tag is for. */
int blsw_pop_verify_batch(const uint8_t* d_pk48, const uint8_t* d_proof96, uint64_t n, int32_t* d_result, int32_t* d_status, void* d_workspace,
                          uint64_t workspace_bytes, void* stream);

/* GROUPED VERIFICATION OVER A MESSAGE TABLE: hash once, one pair per run. New symbols only: the ABI number stays 17 and blsw_engine_options_t is
 * untouched. Many signature sets of a consensus client sign the same message; with blsw_verify_groups_batch or blsw_registry_verify_batch
 * (group >= 1) the caller materialises it n times and the library hashes it, walks its 68 line steps and folds its pair n times. Within a group
 *     prod_{i, m_i = m} e(r_i pk_i, H(m)) = e(sum_i r_i pk_i, H(m)),
 * so the two entries below take the messages as a table with one index per instance and spend one hash per table row and one line chain and one
 * pair per RUN of equal indices.
 *   d_msgs [n_msgs][msg_len]: the table. d_msg_index [n] uint32: instance i signs row d_msg_index[i].
 *   dst: nullable, as in the *_dst entries: NULL is the library's tag and its kernel. There is no second pair of symbols.
 *   Both entries are grouped only: group >= 1 and d_scalars are required (the per-set form gains nothing a gather does not give it). The groups
 *   are exactly those of blsw_verify_groups_batch: instances [g * group, min(n, (g + 1) * group)).
 *   RUNS. Instance i starts a run iff it is the first instance of its group or d_msg_index[i] != d_msg_index[i - 1]; a run is its leader and the
 *   instances up to the next leader or the end of the group. This is a function of (n, group, d_msg_index) alone: statuses and scalars play no
 *   part, and equality is of indices, not of message bytes. Equal indices that are not adjacent are separate runs, which costs time, never
 *   correctness: SORT EACH GROUP BY INDEX.
 *   VERDICT. With P_i = r_i pk_i (the identity for an excluded instance, as in blsw_verify_groups_batch) and R = sum_{i in run} P_i,
 *     d_group_result[g] = 1  iff  every instance of g is included, and  prod_{runs of g} e(R_run, H(d_msgs[idx_run])) * e(-g1, S_g) == 1.
 *   A run whose R is the identity is a skipped pair (factor 1), never zero lines folded in: the rule of an identity S_g.
 *   d_group_runs [ceil(n / group)] uint32 (nullable): the number of runs of each group.
 *   d_status [n][2]: what blsw_verify_groups_batch (respectively blsw_registry_verify_batch) writes, with one rule in front: if
 *   d_msg_index[i] >= n_msgs then [i][0] = BLSW_ST_BAD_INDEX, the instance is excluded, its group is 0 and no table row is read for it.
 *   Every table row is hashed, whether any instance uses it or not.
 * What callers can rest on:
 *   S1. For every input, valid or not, and every choice of scalars, d_group_result and d_status are those of the plain grouped entry on
 *       d_msg[i] = d_msgs[d_msg_index[i]] with the same scalars (all indices in range): the two compute the same element of GT. P1-P4 carry over.
 *   S2. The verdict is invariant under a permutation of the instances of a group (with their scalars and indices); only d_group_runs changes.
 *   S3. d_group_runs is the function stated above.   S4. d_msg_index[i] = i, n_msgs = n: one run per instance.
 * BLSW_ERR_ARG, before any HIP call and with nothing written: the plain grouped entry's conditions (group == 0 included), n_msgs == 0 or
 * > 0x7fffffff, d_msg_index == NULL, a non-NULL dst of length 0, d_msgs == NULL with msg_len != 0. BLSW_ERR_WORKSPACE below the size function,
 * which lays out the plain grouped form over n (points, scaled points, one set of line rows per instance SLOT — the host does not know the runs —
 * group lines, partials), the run arrays (three words per instance, one per group), the run sums (three field elements per slot) and the hash's
 * carve over n_msgs rows, not n, without the latency kernels' buffers (as blsw_verify_pairs_batch). It is non-decreasing in n, n_msgs and msg_len;
 * in `group` it follows the plain layout, whose per-group rows shrink as groups grow.
 * What stays out: the committee form (one committee, a message per slot, nothing shared); blsw_verify_pairs_batch (its pairs belong to one
 * signature and carry no coefficients); merging repeats that are not adjacent (a sort inside the call); a caller's bound on the number of runs
 * that would shrink the line rows. */
int blsw_verify_groups_shared_workspace_bytes(uint64_t n, uint64_t n_msgs, uint32_t msg_len, uint32_t group, uint64_t* bytes);
int blsw_verify_groups_shared_batch(const uint8_t* d_pk48, const uint8_t* d_sig96, const uint8_t* d_msgs, uint32_t msg_len, uint64_t n_msgs,
                                    const uint32_t* d_msg_index, uint64_t n, const uint64_t* d_scalars, uint32_t group, const blsw_dst_t* dst,
                                    int32_t* d_group_result, uint32_t* d_group_runs, int32_t* d_status, void* d_workspace, uint64_t workspace_bytes,
                                    void* stream);
int blsw_registry_verify_shared_workspace_bytes(uint64_t n, uint64_t n_msgs, uint32_t msg_len, uint32_t group, uint64_t* bytes);
int blsw_registry_verify_shared_batch(const blsw_registry_t* r, const uint32_t* d_indices, uint64_t n_indices, const uint64_t* d_offsets,
                                      const uint8_t* d_sig96, const uint8_t* d_msgs, uint32_t msg_len, uint64_t n_msgs, const uint32_t* d_msg_index,
                                      uint64_t n, const uint64_t* d_scalars, uint32_t group, const blsw_dst_t* dst, int32_t* d_group_result,
                                      uint32_t* d_group_runs, int32_t* d_status, uint8_t* d_agg48, void* d_workspace, uint64_t workspace_bytes,
                                      void* stream);

/* Device micro-benchmarks that give the VALU roofline its MEASURED denominator:
 * which = 0: v_mad_u64_u32 rate (32x32+64 multiply-adds per second, all CUs); 1: Fp Montgomery products per second;
 * 2: Fp inversions (safegcd) per second; 3: Fp products per second inside witness-emitting Fp2 mul + sqr;
 * 4: Fp products per second of the 12 x 32-bit CIOS formulation (cross-check of the shipped 14 x 28-bit one). */
int blsw_microbench(int which, uint32_t iters, uint32_t blocks, double* ops_per_s);
/* Same-box yardstick of the HBM roofline: a plain fill of the caller's device buffer (16-byte aligned; overwritten) in the store geometry of the
 * expansion kernel (384 threads x 8 pieces of 16 bytes), `reps` passes after one warm-up pass on the NULL stream of the current device; bytes per
 * second. Boxes of one pool differ by 20-30 % in what they give a write stream: a reader of a bench line needs this next to the kernel's own rate. */
int blsw_fill_rate(void* d_buf, uint64_t bytes, uint32_t reps, double* bytes_per_s);

int blsw_version(void);

#ifdef __cplusplus
}
#endif
#endif
