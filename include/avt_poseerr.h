/* avt_poseerr.h — C ABI of the pose error: how far a fitted avatar is from the avatar that made the data, in metres, part of
 * libavatar_hip.so.  The reference has no counterpart: it never knows the truth.  This engine is developed on synthetic avatars
 * whose generating state is known, and these are the field's standard figures for that comparison: per-vertex error (PVE / V2V),
 * mean per-joint position error (MPJPE), its root-relative form, and the Procrustes-aligned forms (PA-MPJPE, PA-PVE).
 *
 * THE RULE.
 *
 * A scorer is created for point sets of V >= 1 vertices and J >= 0 joints (J == 0: no joint figures) with P = num_parts parts,
 * 1 <= P <= 254, and a table vertex_part[V] with entries in [0, P).  A call compares n pairs (estimate E_i, truth T_i); each side
 * of a pair is a cloud 3 x V and joints 3 x J, column-major doubles: what avt_get_posed returns.  All arithmetic is float64,
 * built without contraction.  Per pair:
 *
 * Vertices.  dx dy dz = E_v - T_v; q_v = (dx*dx + dy*dy) + dz*dz; d_v = sqrt(q_v).  V_SUM = sum d_v, V_SQ = sum q_v, V_MAX = max d_v,
 *   V_ARGMAX the lowest v that attains it.
 * Per part q.  PART_SUM[q], PART_MAX[q] over the vertices with vertex_part[v] == q; an empty part gives 0 and 0.  The part sizes
 *   n_q are constants of the handle (avt_poseerr_part_sizes).
 * Joints (J > 0).  e_j = |E_j - T_j| as d_v above, all J returned; J_SUM, J_MAX, J_ARGMAX.  Root-relative:
 *   r_j = |(E_j - E_0) - (T_j - T_0)|, JR_SUM = sum r_j.  With J == 0 the six joint columns are NaN and J_ARGMAX is -1.
 * Procrustes-aligned figures, for the joints and for the vertices independently.  With x_k the estimate's points and y_k the
 *   truth's: the similarity (s, R, c), R a proper rotation (det R = +1), s >= 0, that minimises sum |s R x_k + c - y_k|^2
 *   (Umeyama 1991 with the reflection correction; computed as Horn's 1987 quaternion form: R is the rotation of the eigenvector
 *   of the largest eigenvalue L of Horn's symmetric 4 x 4 matrix of the centred cross-covariance, s = L / sum |x_k - mean x|^2,
 *   c = mean y - s R mean x).  a_k = |s R (x_k - mean x) - (y_k - mean y)|.  JPA_SUM = sum a_k, JPA_SQ = sum a_k^2 (before the
 *   root), JPA_SCALE = s, and the J aligned errors a_k; VPA_SUM, VPA_SQ, VPA_SCALE for the vertices.
 *   Degenerate estimate: when every x_k equals x_0 (compared with ==: one point, or all coincident), s = 0, R = I: the aligned
 *   estimate is the truth's centroid and a_k = |y_k - mean y|.
 *   Non-unique optimum (the truth's or the estimate's centred points on one line, two points): any minimiser may come back;
 *   *_SQ and *_SCALE are unique there, *_SUM and the per-joint aligned errors need not be.
 * Non-finite input.  A NaN or infinite coordinate in either side of a pair sets AVT_POSEERR_BAD_INPUT in that pair's status word;
 *   the pair's figures are then unspecified (a non-finite point set is not aligned: no other bit is set for it).  The call succeeds
 *   and other pairs are unaffected.
 * Reproducibility.  One workgroup scores one pair, every sum runs in a fixed order, and no floating-point atomic is used: a pair's
 *   results do not depend on n, on the other pairs of the call, on where its inputs came from (host or context), or on the run.
 *   The eigenvalue iteration is cyclic Jacobi with at most AVT_POSEERR_MAX_SWEEPS sweeps; one that has not converged by then sets
 *   AVT_POSEERR_NO_CONVERGENCE and the last iterate is used.
 *
 * Derived figures (ark/PoseError.h derive(), poseerror.metrics): host arithmetic, one division each (and one root):
 *   pve = V_SUM / V   pve_rms = sqrt(V_SQ / V)   pve_part[q] = PART_SUM[q] / n_q (NaN for an empty part)   mpjpe = J_SUM / J
 *   mpjpe_root = JR_SUM / J   pa_mpjpe = JPA_SUM / J   pa_pve = VPA_SUM / V; the maxima and scales are passed through.  Metres.
 * Deliberately not here: thresholds on any figure (nobody has measured what a good fit scores), a per-vertex error download,
 * alignment without scale, and a default place in the tracker's step.
 *
 * Conventions: a handle owns a non-blocking stream on its device; it reads a context's buffers and never writes them.  Functions
 * return 0 on success; avt_last_error() (avt.h) describes a failure.
 */
#ifndef AVT_POSEERR_H_
#define AVT_POSEERR_H_

#ifdef __cplusplus
extern "C" {
#endif

typedef struct avt_poseerr avt_poseerr;
struct avt_model;         /* avt.h */
struct avt_ctx;

/* the columns of a pair's summary row */
enum { AVT_POSEERR_V_SUM = 0, AVT_POSEERR_V_SQ, AVT_POSEERR_V_MAX, AVT_POSEERR_VPA_SUM, AVT_POSEERR_VPA_SQ, AVT_POSEERR_VPA_SCALE,
       AVT_POSEERR_J_SUM, AVT_POSEERR_J_MAX, AVT_POSEERR_JR_SUM, AVT_POSEERR_JPA_SUM, AVT_POSEERR_JPA_SQ, AVT_POSEERR_JPA_SCALE, AVT_POSEERR_COLS };
/* the two sides of a pair; the columns of a pair's argmax row; the bits of its status word */
enum { AVT_POSEERR_ESTIMATE = 0, AVT_POSEERR_TRUTH = 1 };
enum { AVT_POSEERR_V_ARGMAX = 0, AVT_POSEERR_J_ARGMAX = 1 };
enum { AVT_POSEERR_BAD_INPUT = 1, AVT_POSEERR_NO_CONVERGENCE = 2 };
enum { AVT_POSEERR_MAX_SWEEPS = 32 };

/* A scorer of up to max_pairs pairs per call on `device`.  vertex_part: V ints in [0, num_parts); NULL puts every vertex in part
 * 0 and needs num_parts == 1.  Both sides' points and every result of a call live in device memory sized here.  device < 0 makes
 * a host-only handle that checks arguments (upload included: it keeps the count and copies nothing) and refuses to score. */
int avt_poseerr_create(int device, int V, int J, int num_parts, const int* vertex_part, int max_pairs, avt_poseerr** out);
/* The same for a model's V and J with vertex_part[v] = part_map[main joint of v] (avt_model_main_joint: the labelling of
 * renderPartMask and of the optimizer's buckets); part_map: one entry per joint, NULL: the joint itself. */
int avt_poseerr_create_for_model(int device, const struct avt_model* model, int num_parts, const int* part_map, int max_pairs, avt_poseerr** out);
void avt_poseerr_destroy(avt_poseerr* pe);

/* One side of n pairs from the host: clouds n x 3V, joints n x 3J (NULL only if J == 0).  Returns after the copy. */
int avt_poseerr_upload(avt_poseerr* pe, int side, int n, const double* clouds, const double* joints);
/* One side of n pairs from a context on the same device with the same V and J: pair i is frame frames[i] (NULL: i) as the last
 * avt_optimize* / avt_lbs_update left it; indices may repeat and need not be consecutive.  Copied on the device behind the
 * context's queued work and before anything queued on it later; the context is only read and the host does not wait. */
int avt_poseerr_from_ctx(avt_poseerr* pe, int side, struct avt_ctx* ctx, int n, const int* frames);
/* Scores the resident pairs; refuses unless both sides hold the same n >= 1.  Queued on the handle's stream. */
int avt_poseerr_run(avt_poseerr* pe);
/* The result of the last run, after waiting for the handle's stream: summary n x AVT_POSEERR_COLS doubles, per_joint n x 2 x J
 * (raw e_j, then aligned a_j), per_part n x 2 x P (PART_SUM, then PART_MAX), argmax n x 2 ints, status n unsigned ints.  Any
 * pointer may be NULL.  Fails with "no result" when no run succeeded since creation or the last one failed. */
int avt_poseerr_get(avt_poseerr* pe, double* summary, double* per_joint, double* per_part, int* argmax, unsigned int* status, int* n);
/* n_q for q in [0, num_parts); also V, J and num_parts themselves (any pointer may be NULL) */
int avt_poseerr_part_sizes(avt_poseerr* pe, int* sizes, int* V, int* J, int* num_parts);
/* waits for the handle's stream */
int avt_poseerr_sync(avt_poseerr* pe);

#ifdef __cplusplus
}
#endif
#endif
