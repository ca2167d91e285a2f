// Stand-in for the IP data handler (DSCTy 59): never constructed by the golden driver.
#ifndef PACKET_STUB_IP_DATAHANDLER
#define PACKET_STUB_IP_DATAHANDLER
#include "virtual-datahandler.h"
class RadioInterface;
class ip_dataHandler : public virtual_dataHandler {
public:
    ip_dataHandler(RadioInterface *, bool) {}
};
#endif
