// geodesic_lapse_kerr_bl.hip — the KerrBL half of the lapse unit (geodesic_lapse.hip): the
// exact KerrBL trace kernels and geometry buffer fill that also record each hit's coordinate
// time, compiled as geodesic_kerr_bl.hip is, with the machine-level loop-invariant code
// motion off (-mllvm -disable-machine-licm, Makefile).  Built with the standard flags inside
// geodesic_lapse.hip, the KerrBL integrate kernel takes 168 VGPRs and 96 B of scratch per
// lane; built this way it takes the 160 VGPRs and no scratch of grt::kerr_bl's, its sibling
// (DESIGN section 18 has the table).
#define GRT_LAPSE 1
#define GRT_LAPSE_KERR_BL 1
#include "geodesic.hip"
