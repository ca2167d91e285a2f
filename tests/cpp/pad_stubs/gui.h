// Stand-in for the receiver's GUI class: padHandler only connects its signal to it.
#ifndef PAD_STUB_GUI
#define PAD_STUB_GUI
class RadioInterface {};
#endif
