// fused decomposing external-product kernel instantiations: native kind 4
#define INST_KIND 4
#include "native_gadget_inst.inc"
