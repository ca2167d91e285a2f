// Stand-in for the journaline data handler (DSCTy 44): never constructed by the golden driver.
#ifndef PACKET_STUB_JOURNALINE_DATAHANDLER
#define PACKET_STUB_JOURNALINE_DATAHANDLER
#include "virtual-datahandler.h"
class journaline_dataHandler : public virtual_dataHandler {
public:
    journaline_dataHandler() {}
};
#endif
