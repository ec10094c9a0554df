// ThreadGrid.h -- the occupancy-grid worker; public surface of the reference's ThreadGrid (src/ThreadGrid.h:24-129,
// src/ThreadGrid.cpp).  Every wake-up publishes one frame of the device (tsd_map_frame_begin / _wait: the occupancy map and the
// colour image from one pass over the tiles) on <node>/map and <node>/map/image; <node>/get_map answers with the last map.
#pragma once
#include <cstdint>
#include <memory>
#include <mutex>

#include "ThreadSLAM.h"
#include "ros_shim.h"

namespace ohm_tsd_slam
{

class ThreadGrid : public ThreadSLAM
{
public:
  ThreadGrid(obvious::TsdGrid* grid, const std::shared_ptr<rclcpp::Node>& node, const double xOffset, const double yOffset);
  virtual ~ThreadGrid();

  /** one publication on the caller's thread, what every wake-up of the event loop does (not in the reference: deterministic tests).
   *  Returns TSD_OK or the frame's error code. */
  int publish(void);
  /** frames published so far */
  uint64_t frames(void);

  std::shared_ptr<rclcpp::Publisher<nav_msgs::msg::OccupancyGrid>> gridPublisher() { return _gridPub; }
  std::shared_ptr<rclcpp::Publisher<sensor_msgs::msg::Image>> imagePublisher() { return _pubColorImage; }
  std::shared_ptr<rclcpp::Service<nav_msgs::srv::GetMap>> mapService() { return _getMapServ; }

  /** the get_map service (ThreadGrid.cpp:135-142): the last map with a fresh stamp */
  bool getMapServCallBack(const std::shared_ptr<nav_msgs::srv::GetMap::Request> req,
                          std::shared_ptr<nav_msgs::srv::GetMap::Response> res);

protected:
  virtual void eventLoop(void);

private:
  std::shared_ptr<rclcpp::Node> _node;
  std::shared_ptr<nav_msgs::msg::OccupancyGrid> _occGrid;
  sensor_msgs::msg::Image _image;
  std::shared_ptr<rclcpp::Service<nav_msgs::srv::GetMap>> _getMapServ;
  std::shared_ptr<rclcpp::Publisher<nav_msgs::msg::OccupancyGrid>> _gridPub;
  std::shared_ptr<rclcpp::Publisher<sensor_msgs::msg::Image>> _pubColorImage;
  unsigned int _width;
  unsigned int _height;
  double _cellSize;
  unsigned int _objInflateFactor;
  bool _objectInflation;
  // page-locked landing buffers of the frames (the persistent _occGridContent lives on the device)
  int8_t* _hOcc;
  uint8_t* _hRgb;
  std::mutex _publishMutex;      // one publication at a time (event loop, publish())
  std::mutex _msgMutex;          // _occGrid between a publication and the get_map service
  uint64_t _frames;
};

} /* namespace ohm_tsd_slam */
