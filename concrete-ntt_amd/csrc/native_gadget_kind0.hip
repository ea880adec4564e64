// fused decomposing external-product kernel instantiations: native kind 0
#define INST_KIND 0
#include "native_gadget_inst.inc"
