/* avt_render.h — C ABI of the avatar renderer on the GPU, part of libavatar_hip.so.
 *
 * The overlay stage of the reference's tracking loop: `ark::AvatarRenderer` (AvatarRenderer.h, AvatarRenderer.cpp:11-224,
 * AvatarHelpers.cpp:61-303) for avatars that are already posed.  Every output is the reference's, pixel for pixel:
 *
 *   projection     (float)(x * fx / z + cx), (float)(-y * fy / z + cy) in double, fx..cy floats (Calibration.h:13)  (:11-37)
 *   painter order  faces by decreasing mean depth (float)((za + zb + zc) / 3.f); equal keys by ascending face id (the
 *                  reference's std::sort leaves them unspecified)                                                  (:39-70)
 *   depth          float, 0 = background; |n_z| < 0.1 paints 0 with the end-exclusive row fill, the others the
 *                  barycentric row fill of z clamped to [0, 255]                                                    (:72-101)
 *   part mask      uint8, 255 = background; |n_z| < 0.1 paints 255, the others the column fill labelled by the nearest
 *                  projected vertex, label = part_map[assignedJoints[v][0]] (joint id without a part map)          (:174-202)
 *   Lambert        uint8, 0 = background; per-vertex normals summed over the incident faces in painter order, then
 *                  divided by their norm with no zero guard and turned to face the camera; two lights in double; only
 *                  faces with |n_z| > 1e-2 are painted, with the barycentric row fill; x86 float -> uint8 (NaN -> 0)
 *                                                                                                                   (:104-172)
 *   faces          int32, -1 = background; every face paints its painter position with the end-exclusive row fill  (:204-217)
 *
 * A handle holds up to max_images posed avatars of one model and renders them with one launch sequence on its own
 * non-blocking stream.  The avatars come either from the host (avt_renderer_upload) or from the frames of a context after
 * avt_optimize* (avt_renderer_from_ctx: copied on the device, after the context's queued work, with no host round trip;
 * the context's buffers are only read).  Clouds are 3 x V column-major doubles (ava.cloud: x, y, z per vertex), joints
 * 3 x J.  Functions return 0 on success; avt_last_error() (avt.h) describes a failure.
 */
#ifndef AVT_RENDER_H_
#define AVT_RENDER_H_

#include "avt.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct avt_renderer avt_renderer;

/* what avt_renderer_run renders (any combination; 0 = projections and painter order only) */
enum { AVT_RENDER_DEPTH = 1, AVT_RENDER_PART_MASK = 2, AVT_RENDER_LAMBERT = 4, AVT_RENDER_FACES = 8 };

/* AvatarRenderer(ava, intrin): a renderer for avatars of model m on `device`, images of width x height. */
int avt_renderer_create(int device, const avt_model* m, int width, int height, float fx, float fy, float cx, float cy, int max_images,
                        avt_renderer** out);
void avt_renderer_destroy(avt_renderer* r);

/* renderPartMask's part_map: part of joint j (n_joints entries; NULL or 0 entries: the joint id itself). */
int avt_renderer_set_part_map(avt_renderer* r, int n_joints, const int* part_map);

/* n_images posed avatars from the host: clouds n x 3 x V, joints n x 3 x J (NULL: no joints, avt_renderer_projection
 * then refuses joints_2xJ). */
int avt_renderer_upload(avt_renderer* r, int n_images, const double* clouds, const double* joints);

/* n_images posed avatars from context c (same model, same device): image i is frame frames[i] (NULL: frame i) as
 * avt_get_posed would return it, cloud and joints. */
int avt_renderer_from_ctx(avt_renderer* r, avt_ctx* c, int n_images, const int* frames);

/* queues the projections, the painter order and the images selected by `what` (AVT_RENDER_*) for every resident avatar */
int avt_renderer_run(avt_renderer* r, int what);

/* waits for the run and copies image `image` out; any pointer may be NULL; an image the last run did not render is refused.
 * depth: height x width float32, part_mask / lambert: uint8, faces: int32. */
int avt_renderer_download(avt_renderer* r, int image, float* depth, unsigned char* part_mask, unsigned char* lambert, int* faces);

/* waits for the run and copies the rest of image `image` out; any pointer may be NULL.
 * points_2xV / joints_2xJ: projected (x, y) per vertex / joint (getProjectedPoints / getProjectedJoints);
 * face_keys / faces_3xF: getOrderedFaces, the sort key and the vertex triple of every face in painter order;
 * face_pos: painter position of every face (face id order). */
int avt_renderer_projection(avt_renderer* r, int image, float* points_2xV, float* joints_2xJ, float* face_keys, int* faces_3xF,
                            int* face_pos);

/* waits for the run and copies renderLambert's per-vertex values of image `image` out (the last run must have rendered the
 * Lambert image); either pointer may be NULL.  normals_3xV: the vertex normals as the shading uses them (incident face normals
 * summed in painter order, divided by their norm - NaN for a zero sum -, turned to face the camera); lambert_v: the per-vertex
 * value std::max(float(...) * 255, 0.f) that the fill interpolates. */
int avt_renderer_vertex_shading(avt_renderer* r, int image, double* normals_3xV, float* lambert_v);

/* waits for the handle's stream */
int avt_renderer_sync(avt_renderer* r);

/* painter-order algorithm: 0 = per-image sort in LDS (default), 1 = the O(F^2) rank count; both give the same positions */
int avt_renderer_set_ordering(avt_renderer* r, int ordering);

#ifdef __cplusplus
}
#endif
#endif
