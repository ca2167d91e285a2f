// Stand-in for the receiver's GUI class: the data-group handler only keeps a pointer to it.
#ifndef PACKET_STUB_GUI
#define PACKET_STUB_GUI
class RadioInterface {};
#endif
