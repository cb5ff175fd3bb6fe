// geodesic_seq.hip — the exact trace kernels (integrate, tail, shade, raymarch) and the
// work-order probes of every chart, built once more for camera sequences
// (grt_render_sequence): K frames of one scene stacked into one rectangle of K * rows rows
// and traced as one work queue.  Same source, same flags and the same arithmetic as
// geodesic.hip (-ffp-contract=off), so each frame's pixels are bit-identical to rendering
// its camera alone; the one difference is where a ray's camera comes from: the entry of
// its frame in a device table (CamTable, kernels.h), picked per lane from the integer
// stacked row, instead of DevScene::cam.  The tile queue, the output slots, the workspace,
// the hit pool, offset lists, the tail hand-off and the raymarch work on the stacked
// rectangle as they do on any other.  The table is an extra parameter of this unit's
// kernels, so the kernels of the other units are compiled from unchanged code.
// grt_set_arithmetic(1) does not apply here: there is no fused sequence unit.
#define GRT_SEQ 1
#include "geodesic.hip"
